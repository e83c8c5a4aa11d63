"""Tensor-level wrappers over the C ABI (include/mi_ddpm.h).

Activations are fp32 NHWC tensors [N, H, W, C] on a HIP device; a channel slice
``t[..., a:b]`` of a contiguous tensor is a legal activation (pixel stride ld = t.stride(2)).
Every function launches on torch's current stream and never synchronises.  There is no
CPU path: a tensor that is not on a GPU raises.

Shape questions (`*_supported`, `*_tile`, `*_picked`, workspace sizes) are answered once per shape and kept in _QUERY_CACHE, the only
cache here: a library query goes through `_query`, Python logic around queries carries `@_cached_question`.  Their arguments are
numbers and tuples of numbers; a launch wrapper is never cached.  `_QUERY_CACHE.clear()` follows any debug hook of the library and
any rebinding of a module switch (PW_MIN_TILES, USE_*) that an answer depends on.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

from .lib import ROWSUM_MAX, WGRAD_STORE, MiConvDesc, MiGnDesc, MiRowSum, MiWgradDesc, check, load_library

MODE_FP32, MODE_BF16 = 0, 1


def debug_knob(name: str, default: str) -> str:
    """Experiment / A-B switches (kernel picks, copies on or off): honoured only when MI_DEBUG_KNOBS=1 is set as well (the tools/
    that A/B them, e.g. tools/sample_steps.py, set it), so that a stray variable cannot put a production run on a path the test suite does not cover.  The mode selectors a
    user is meant to set are read directly: MI_DDPM_MODE, MI_DDPM_STORAGE, MI_DDPM_FUSE_GN, MI_DDPM_GRAPH, MI_DDPM_LIB,
    MI_CONV_AUTO (halo-only fallback, covered by a subprocess test), MI_DDP_BUCKET_MB, MI_DIST_BACKEND."""
    if os.environ.get("MI_DEBUG_KNOBS") == "1":
        return os.environ.get(name, default)
    return default
PROBE = None      # bench.py sets this to a list: (kernel symbol, algorithmic FLOPs, start event, end event, shape note, algorithmic
                  # HBM bytes) per launch, events recorded on the launch stream


# MI_CONV_AUTO=0: the register-staged halo kernel (round 1 / 2) everywhere -- the fallback of the per-layer pick below, kept under test
# by a subprocess run of the conv and UNet tests.
CONV_AUTO = os.environ.get("MI_CONV_AUTO", "1") == "1"


# The private-weight-stream kernel (csrc/conv_pw.hip): 128-pixel tiles, one barrier per 64-channel chunk, two workgroups per CU.
USE_CONV_PW = CONV_AUTO and debug_knob("MI_CONV_PW", "1") == "1"     # MI_CONV_AUTO=0: the halo kernel everywhere


def _pw_sym(d, out16, var=0):
    """conv_pw_kernel's symbol as rocprofv3 prints it."""
    pt = _query("mi_conv3x3_pw_tile", d) if var < 2 else 128
    pt = _pw_tile_now(d, var, False, pt)
    return f"conv_pw_kernel<{'true' if out16 else 'false'}, {var}, 0, {pt or 128}>"


def _pw_tile_now(d, var, in32, pt):
    """The tile a launch runs on right now: a split-K launch (mi_conv3x3_pw_splitk) takes 128-pixel tiles where the unsplit rule takes 64."""
    q = _query("mi_conv3x3_pw_splitk", d, var, int(in32))
    return (q >> 4) if (q & 15) > 1 else pt


def _pick_pw(N, H, W, K, Nc, d=None):
    """The private-weight-stream kernel takes a layer that offers it at least about one tile per CU: 128-pixel x 128-channel tiles,
    or (d given: the plain conv and the variant with GroupNorm sums; the library decides, mi_conv3x3_pw_tile) 64-pixel tiles when
    the 128-pixel ones would be too few.  Smaller layers stay with round 2's kernels."""
    pt = 128
    if d is not None:
        pt = _query("mi_conv3x3_pw_tile", d)
        if not pt:
            return False
    return (N * H * W // pt) * ((Nc + 127) // 128) >= PW_MIN_TILES


PW_MIN_TILES = int(debug_knob("MI_CONV_PW_MIN_TILES", "64"))


USE_WGRAD_TR = debug_knob("MI_W3_TR", "1") != "0"      # A/B switch for the LDS-DMA weight-gradient kernel (csrc/wgrad_tr.hip)


_QUERY_CACHE, _MISSING = {}, object()


def _desc_key(d):
    return tuple(getattr(d, f) for f, _ in d._fields_)


def _query(name, *args):
    """Cached answer (yes / no, tile, size) of a library query, keyed by its arguments' values (a descriptor: its fields).  The answers
    are pure functions of them, and one FFI call per launch for them was ~15 % of the step's enqueue time."""
    key = (name, *[_desc_key(a) if isinstance(a, C.Structure) else a for a in args])
    r = _QUERY_CACHE.get(key, _MISSING)
    if r is _MISSING:
        r = _QUERY_CACHE[key] = getattr(load_library(), name)(*[C.byref(a) if isinstance(a, C.Structure) else a for a in args])
    return r


def _cached_question(fn):
    """A shape question written in Python: evaluated once per (name, positional, sorted keyword arguments), kept in _QUERY_CACHE.
    A tensor among the arguments is a TypeError: what takes tensors launches, and a launch is never answered from a cache."""
    name = fn.__name__

    def ask(*args, **kw):
        key = (name, args, tuple(sorted(kw.items()))) if kw else (name, args)
        r = _QUERY_CACHE.get(key, _MISSING)
        if r is _MISSING:
            if any(isinstance(x, torch.Tensor) for a in (*args, *kw.values()) for x in (a if isinstance(a, tuple) else (a,))):
                raise TypeError(f"{name}: a cached shape question takes numbers and tuples of numbers, not tensors")
            r = _QUERY_CACHE[key] = fn(*args, **kw)
        return r
    ask.__name__, ask.__qualname__, ask.__doc__, ask.__wrapped__ = name, fn.__qualname__, fn.__doc__, fn
    return ask


def _conv_desc(N, H, W, K, Nc, k, *, out_hw=None, stride=1, pad=None, transposed=False, w_kn=False, mode=MODE_BF16, K1=None, ldx=None,
               ldx2=0, ldy=None, ldr=0, accumulate=False):
    """MiConvDesc of a k x k (or k = (kh, kw)) conv on an H x W input.  Unless told otherwise: stride 1, pad k // 2, output of the same
    size, bf16 mode, one dense source (K1 = ldx = K, ldx2 = 0), dense output (ldy = Nc), no residual, no accumulate."""
    OH, OW = (H, W) if out_hw is None else out_hw
    kh, kw = k if isinstance(k, tuple) else (k, k)
    return MiConvDesc(N, H, W, OH, OW, K, Nc, kh, kw, stride, kh // 2 if pad is None else pad, int(transposed), int(w_kn), mode,
                      K if K1 is None else K1, K if ldx is None else ldx, ldx2, Nc if ldy is None else ldy, ldr, int(accumulate))


def _wgrad_desc(N, grid_g, grid_d, Ci, Cj, k, stride, pad, gather_i, mode, ldp, ldq, I1=None, ldp2=0):
    """MiWgradDesc: the gathered operand on grid_g = (H, W), the other on grid_d; k x k (or k = (kh, kw)); P in one piece unless I1, ldp2."""
    kh, kw = k if isinstance(k, tuple) else (k, k)
    return MiWgradDesc(N, grid_g[0], grid_g[1], grid_d[0], grid_d[1], Ci, Cj, kh, kw, stride, pad, int(gather_i), mode, Ci if I1 is None else I1, ldp, ldp2, ldq)


def _ldn(t) -> int:
    return 0 if t is None else ld_of(t)


@_cached_question
def _linattn_ws(N, n, heads):
    return load_library().mi_linattn_workspace(N, n, heads)


@_cached_question
def _cvt_colsum_ws(M, Cc):
    return load_library().mi_f32_to_bf16_colsum_workspace(M, Cc)


def _probe_open():
    if PROBE is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _probe_close(e0, sym, flops, desc, nbytes=0.0):
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROBE.append((sym, float(flops), e0, e1, desc, float(nbytes)))


def _esz(t) -> int:
    return 0 if t is None else t.element_size()


def _stream() -> C.c_void_p:
    """torch's current stream on the CURRENT device: kernels launch on the current HIP device, so every wrapper first checks
    (`_need_gpu`) that its tensors live there -- a rank that forgot `torch.cuda.set_device(LOCAL_RANK)` raises instead of
    launching on GPU 0 against another GPU's memory."""
    global LAUNCHES
    LAUNCHES += 1
    return C.c_void_p(_raw_stream(_cur_dev()))


def _count_launches(more: int):
    """A library call that launches several kernels adds the ones behind its first (the pair head: its tests pin the kernel count)."""
    global LAUNCHES
    LAUNCHES += more


LAUNCHES = 0      # library launches so far (every wrapper fetches the stream once per launch): lets a stream capture know whether a
                  # segment it is about to close recorded anything (src/runtime/graphed.py)


# the raw forms of torch.cuda.current_device() / current_stream(): same answers (they follow torch.cuda.stream(...) contexts and
# graph capture), without the Python-side device bookkeeping that cost ~3 us per launch
_cur_dev = torch._C._cuda_getDevice
_raw_stream = torch._C._cuda_getCurrentRawStream


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _need_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"expected float32 (or bf16 block-internal storage), got {t.dtype}")
    if t.device.index != _cur_dev():
        raise RuntimeError(f"tensor is on {t.device} but the current HIP device is cuda:{torch.cuda.current_device()}; "
                           "call torch.cuda.set_device(tensor.device) first (one process per GPU)")
    if t.device.index not in _SPLITK_WS:
        _splitk_workspace(t.device)


# Split-K launches of the 3x3 tile kernel (the layers whose tiles would leave CUs without a workgroup: the sampler at B = 64, cfg 3 at 32 images
# per GPU) exchange fp32 partial tiles through a per-device workspace the library is told about once: zeroed here, never freed (captured graphs
# hold its address).  SPLITK_MB = 0 (MI_CONV_PW_SPLITK_MB with MI_DEBUG_KNOBS=1) leaves every launch unsplit.
_SPLITK_WS = {}
SPLITK_MB = int(debug_knob("MI_CONV_PW_SPLITK_MB", "64"))


def _splitk_workspace(device):
    ws = None
    if SPLITK_MB > 0 and USE_CONV_PW and not torch.cuda.is_current_stream_capturing():
        ws = torch.zeros(SPLITK_MB << 20, dtype=torch.uint8, device=device)
        torch.cuda.current_stream().synchronize()
        check(load_library().mi_conv_pw_set_splitk_workspace(ws.data_ptr(), ws.numel()), "mi_conv_pw_set_splitk_workspace")
    elif torch.cuda.is_current_stream_capturing():
        return                                   # decided by the first eager call on this device
    _SPLITK_WS[device.index] = ws


def ld_of(t: torch.Tensor) -> int:
    """Pixel stride of an NHWC activation (or row stride of a 2-D [M, C] matrix)."""
    if t.dim() == 2:
        assert t.stride(1) == 1
        return t.stride(0)
    n, h, w, c = t.shape
    ld = t.stride(2)
    assert t.stride(3) == 1 and ld >= c, (t.shape, t.stride())
    assert (w == 1 or True) and t.stride(1) == w * ld and (n == 1 or t.stride(0) == h * w * ld), (t.shape, t.stride())
    return ld


def new_act(n, h, w, c, like: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return torch.empty((n, h, w, c), device=like.device, dtype=dtype)


def _b16(t) -> int:
    return int(t is not None and t.dtype == torch.bfloat16)


# --------------------------------------------------------------------------- conv family
@_cached_question
def igemm_bf16_in_supported(K, Nc, k, stride, transposed, mode, out_hw):
    """Can conv_igemm read bf16-stored activations for this layer (the stride-2 conv / transposed conv family, dense tensors)?"""
    return bool(_query("mi_conv_igemm_bf16w_io_supported", _conv_desc(1, 1, 1, K, Nc, k, out_hw=out_hw, stride=stride, pad=1, transposed=transposed, mode=mode)))


USE_CONV_GT = debug_knob("MI_CONV_GT", "1") != "0"      # A/B switch: the tap-gather kernel for the stride-2 / transposed convs


def conv_gt(x, wq, *, kh, kw, stride, pad, transposed, K, Nc, out_hw, bias=None, residual=None, out=None, accumulate=False,
            out_dtype=torch.float32, mode=MODE_BF16, want16=False):
    """The stride-2 / transposed convs and their data gradients through the tap-gather kernel (mi_conv_gt): x bf16, wq = the layer's
    fragment-order weights (wfq: contraction over the master layout's ci, wdq: over co).  Returns None when the kernel does not take
    the layer (the caller falls back to conv_igemm).  mode = MODE_FP32: the exact-fp32 instantiation (x fp32, wq = wfq32 / wdq32)."""
    if not USE_CONV_GT or wq is None or x.dtype != (torch.bfloat16 if mode == MODE_BF16 else torch.float32):
        return None
    _need_gpu(x)
    N, IH, IW, _ = x.shape
    OH, OW = out_hw
    d = _conv_desc(N, IH, IW, K, Nc, (kh, kw), out_hw=out_hw, stride=stride, pad=pad, transposed=transposed, mode=mode, ldx=ld_of(x),
                   ldy=Nc if out is None else ld_of(out), ldr=_ldn(residual), accumulate=accumulate)
    if d.ldy % 8 or not _query("mi_conv_gt_supported", d):
        return None
    if out is None:
        assert not accumulate
        out = new_act(N, OH, OW, Nc, x, out_dtype)
        d.ldy = ld_of(out)
    e0 = _probe_open()
    y16 = None
    if want16:          # -> (y, y16): the bf16 copy of the fp32 output from the same epilogue
        assert out.dtype == torch.float32 and not accumulate and mode == MODE_BF16
        y16 = new_act(N, OH, OW, Nc, x, torch.bfloat16)
        check(load_library().mi_conv_gt_dual(C.byref(d), _p(x), _p(wq), _p(bias), _p(residual), _p(out), _p(y16), ld_of(y16), _stream()),
              "mi_conv_gt_dual")
    else:
        check(load_library().mi_conv_gt(C.byref(d), _p(x), _p(wq), _p(bias), _p(residual), _p(out), _b16(out), _stream()), "mi_conv_gt")
    if e0 is not None:
        pxt, ncls = C.c_int(), C.c_int()
        load_library().mi_conv_gt_tile(C.byref(d), C.byref(pxt), C.byref(ncls))
        flops = 2.0 * N * OH * OW * Nc * K * (kh * kw if not (transposed and stride > 1) else kh * kw / (stride * stride))
        nb = N * IH * IW * K * _esz(x) + N * OH * OW * Nc * _esz(out) * (2 if accumulate else 1) + kh * kw * K * Nc * _esz(x)
        _probe_close(e0, f"conv_gt_kernel<{'true' if _b16(out) else 'false'}, {pxt.value}{', true' if mode == MODE_FP32 else ''}>", flops,
                     f"N{N} {IH}x{IW}->{OH}x{OW} K{K}->{Nc} k{kh} s{stride} T{int(transposed)} acc{int(accumulate)}", nb)
    return (out, y16) if want16 else out


def conv_igemm(x, w, *, kh, kw, stride, pad, transposed, w_kn, K, Nc, out_hw, mode, x2=None,
               bias=None, residual=None, out=None, accumulate=False, wb=None):
    """y = conv(x [| x2]) per MiConvDesc.  x: [N,IH,IW,K1], x2: [N,IH,IW,K-K1] or None."""
    _need_gpu(x)
    N, IH, IW, K1 = x.shape
    if x2 is None:
        K1 = K
    OH, OW = out_hw
    if out is None:
        assert not accumulate
        out = new_act(N, OH, OW, Nc if Nc % 4 == 0 else (Nc + 3) // 4 * 4, x)
        if out.shape[3] != Nc:
            out.zero_()
            out = out[..., :Nc]
    d = _conv_desc(N, IH, IW, K, Nc, (kh, kw), out_hw=out_hw, stride=stride, pad=pad, transposed=transposed, w_kn=w_kn, mode=mode, K1=K1,
                   ldx=ld_of(x), ldx2=_ldn(x2), ldy=ld_of(out), ldr=_ldn(residual), accumulate=accumulate)
    if PROBE is not None:
        bm, bn = C.c_int(), C.c_int()
        load_library().mi_conv_igemm_tile(C.byref(d), C.byref(bm), C.byref(bn))
        flops = 2.0 * N * OH * OW * Nc * K * (kh * kw if not (transposed and stride > 1) else kh * kw / (stride * stride))
        e0 = _probe_open()
    in16 = _b16(x)
    if in16:                                                     # bf16-stored activations: ring kernel with 64-channel stages
        if wb is None or mode != MODE_BF16 or (x2 is not None and not _b16(x2)) or not load_library().mi_conv_igemm_bf16w_io_supported(C.byref(d)):
            raise RuntimeError("bf16-stored activations: layer not supported (check igemm_bf16_in_supported first)")
        check(load_library().mi_conv_igemm_bf16w_io(C.byref(d), _p(x), _p(x2), _p(wb), _p(bias), _p(residual), _p(out), 1, _stream()),
              "mi_conv_igemm_bf16w_io")
    elif wb is not None and mode == MODE_BF16 and K % 8 == 0:    # bf16 weight copy [tap][Nc][K]
        check(load_library().mi_conv_igemm_bf16w(C.byref(d), _p(x), _p(x2), _p(wb), _p(bias), _p(residual), _p(out), _stream()),
              "mi_conv_igemm_bf16w")
    else:
        check(load_library().mi_conv_igemm(C.byref(d), _p(x), _p(x2), _p(w), _p(bias), _p(residual), _p(out), _stream()),
              "mi_conv_igemm")
    if PROBE is not None:
        fast = wb is not None and mode == MODE_BF16 and K % 8 == 0
        nb = N * IH * IW * K * _esz(x) + N * OH * OW * Nc * _esz(out) * (2 if accumulate else 1) + kh * kw * K * Nc * (2 if fast else 4)
        _probe_close(e0, f"igemm{'_fast' if fast else ''}_kernel<{mode},{bm.value},{bn.value}{',in16' if in16 else ''}>", flops,
                     f"N{N} {IH}x{IW}->{OH}x{OW} K{K}->{Nc} k{kh} s{stride} T{int(transposed)} acc{int(accumulate)}", nb)
    return out


def conv3x3_bf16w(x, wsh, *, K, Nc, flip, ksize=3, x2=None, bias=None, residual=None, out=None, accumulate=False,
                  out_dtype=torch.float32, gn_sums=None, want16=False, wq=None):
    """3x3/s1/p1 (or 1x1) conv (flip=False) or its data gradient (flip=True) through the pipelined
    LDS-tile kernel.  wsh: bf16 weights [k][k][Nc][K].  Returns None when the shape is not supported.
    want16: -> (y, y16), the fp32 output and its bf16 copy written by the same epilogue.
    wq: the same weights in MFMA-fragment order (pack_weights_bf16's wfq / wdq slice) -- lets the private-weight-stream kernel
    (mi_conv3x3_pw) take the layer."""
    _need_gpu(x)
    N, H, W, K1 = x.shape
    if x2 is None:
        K1 = K
    d = _conv_desc(N, H, W, K, Nc, ksize, transposed=flip, K1=K1, ldx=ld_of(x), ldx2=_ldn(x2), ldy=0, ldr=_ldn(residual), accumulate=accumulate)
    lib = load_library()
    if not _query("mi_conv3x3_bf16w_supported", d):
        return None
    if out is None:
        assert not accumulate
        out = new_act(N, H, W, Nc, x, out_dtype)
    d.ldy = ld_of(out)
    io = _b16(x) | (_b16(out) << 1)
    assert x2 is None or x2.dtype == x.dtype
    pick = "halo"
    if (ksize == 1 and wq is not None and USE_CONV_PW and _b16(x) and gn_sums is None and K % 128 == 0
            and _query("mi_conv1x1_pw_supported", d)):
        # the streaming 1x1 kernel: tile by LDS-DMA per 128-channel chunk, per-wave weight fragments, whole-row stores (conv1x1_pw_kernel)
        y16 = new_act(N, H, W, Nc, x, torch.bfloat16) if want16 else None
        assert not (want16 and (accumulate or _b16(out)))
        e0 = _probe_open()
        check(lib.mi_conv1x1_pw(C.byref(d), _p(x), _p(x2), _p(wq), _p(bias), _p(residual), _p(out), _b16(out), _p(y16),
                                ld_of(y16) if y16 is not None else 0, _stream()), "mi_conv1x1_pw")
        if e0 is not None:
            nb = (N * H * W * K * 2 + N * H * W * Nc * (_esz(out) * (2 if accumulate else 1) + _esz(residual) + (2 if want16 else 0)) + K * Nc * 2)
            px = 64 if (N * H * W // 128) * ((Nc + 127) // 128) < 256 else 128
            # (the channel-tile loop instantiation: mi_conv1x1_pw's condition, restated for the symbol name only)
            sw = lib.mi_debug_conv1x1_pw_nloop(-1)
            nloop = (_b16(out) and residual is None and not accumulate and px == 128 and K == 128 and x2 is None and Nc > 128
                     and (sw == 2 or (sw == 1 and N * H * W // 128 >= 1024)))
            sym = (f"conv1x1_pw_kernel<true, false, 128, false, false, true>" if nloop else
                   f"conv1x1_pw_kernel<{'true' if _b16(out) else 'false'}, {'true' if want16 else 'false'}, {px}>")
            _probe_close(e0, sym, 2.0 * N * H * W * Nc * K,
                         f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} flip{int(flip)} acc{int(accumulate)}", nb)
        return (out, y16) if want16 else out
    if (ksize == 1 and not _b16(x) and USE_CONV_PW and wq is not None and not want16 and gn_sums is None and K % 128 == 0
            and _query("mi_conv1x1_pw_x32_supported", d)):
        # fp32-stored input of a 1x1 conv (the residual-stream gradient of to_out / res_conv's data gradients, res_conv in inference)
        e0 = _probe_open()
        check(lib.mi_conv1x1_pw_x32(C.byref(d), _p(x), _p(x2), _p(wq), _p(bias), _p(residual), _p(out), _b16(out), _stream()), "mi_conv1x1_pw_x32")
        if e0 is not None:
            nb = (N * H * W * K * 4 + N * H * W * Nc * (_esz(out) * (2 if accumulate else 1) + _esz(residual)) + K * Nc * 2)
            _probe_close(e0, f"conv1x1_pw_kernel<{'true' if _b16(out) else 'false'}, false, 64, false, true>", 2.0 * N * H * W * Nc * K,
                         f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} fp32 in flip{int(flip)} acc{int(accumulate)}", nb)
        return out
    if (ksize == 3 and not _b16(x) and USE_CONV_PW and wq is not None and not want16 and d.ldx % 4 == 0 and (x2 is None or d.ldx2 % 4 == 0)):
        # fp32-stored input (the residual stream: the sampler's block1 convs): the same kernel, pieces rounded to bf16 while staged
        pt = _query("mi_conv3x3_pw_x32_tile", d)
        if pt and (N * H * W // pt) * ((Nc + 127) // 128) >= PW_MIN_TILES:
            assert gn_sums is None or (gn_sums.dtype == torch.int64 and gn_sums.numel() == N * (Nc // 16) * 2)
            e0 = _probe_open()
            check(lib.mi_conv3x3_pw_x32(C.byref(d), _p(x), _p(x2), _p(wq), _p(bias), _p(residual), _p(out), _b16(out), _p(gn_sums), _stream()),
                  "mi_conv3x3_pw_x32")
            if e0 is not None:
                nb = (N * H * W * K * 4 + N * H * W * Nc * (_esz(out) * (2 if accumulate else 1) + _esz(residual)) + 9 * K * Nc * 2)
                _probe_close(e0, f"conv_pw_kernel<{'true' if _b16(out) else 'false'}, {0 if gn_sums is None else 1}, 0, {_pw_tile_now(d, 0, True, pt)}, true>",
                             2.0 * N * H * W * Nc * K * 9, f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} fp32 in flip{int(flip)} acc{int(accumulate)}", nb)
            return out
    if (gn_sums is not None and ksize == 3 and _b16(x) and USE_CONV_PW and wq is not None and _pick_pw(N, H, W, K, Nc, d)
            and _query("mi_conv3x3_pw_supported", d)):
        # the next layer's GroupNorm sums from the private-weight-stream kernel's epilogue
        assert gn_sums.dtype == torch.int64 and gn_sums.numel() == N * (Nc // 16) * 2
        e0 = _probe_open()
        check(lib.mi_conv3x3_pw_gnsums(C.byref(d), _p(x), _p(x2), _p(wq), _p(bias), _p(residual), _p(out), _b16(out), _p(gn_sums), _stream()),
              "mi_conv3x3_pw_gnsums")
        if e0 is not None:
            nb = (N * H * W * K * 2 + N * H * W * Nc * (_esz(out) * (2 if accumulate else 1) + _esz(residual)) + 9 * K * Nc * 2)
            _probe_close(e0, _pw_sym(d, _b16(out), 1), 2.0 * N * H * W * Nc * K * 9,
                         f"N{N} {H}x{W} K{K}->{Nc} + GroupNorm sums", nb)
        return out
    if gn_sums is None and not want16 and ksize == 3 and _b16(x):
        if USE_CONV_PW and wq is not None and _pick_pw(N, H, W, K, Nc, d):
            pick = "pw"
    if pick == "pw":
        e0 = _probe_open()
        check(lib.mi_conv3x3_pw(C.byref(d), _p(x), _p(x2), _p(wq), _p(bias), _p(residual), _p(out), _b16(out), _stream()), "mi_conv3x3_pw")
        if e0 is not None:
            nb = (N * H * W * K * 2 + N * H * W * Nc * (_esz(out) * (2 if accumulate else 1) + _esz(residual)) + 9 * K * Nc * 2)
            _probe_close(e0, _pw_sym(d, _b16(out)), 2.0 * N * H * W * Nc * K * 9,
                         f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} flip{int(flip)} acc{int(accumulate)}", nb)
        return out
    e0 = _probe_open()
    if want16:                    # fp32 output + its bf16 copy from one epilogue
        assert out.dtype == torch.float32 and gn_sums is None and not accumulate
        y16 = new_act(N, H, W, Nc, x, torch.bfloat16)
        check(lib.mi_conv3x3_bf16w_io_dual(C.byref(d), _p(x), _p(x2), _p(wsh), _p(bias), _p(residual), _p(out), _p(y16), ld_of(y16), io, _stream()),
              "mi_conv3x3_bf16w_io_dual")
    elif gn_sums is not None:     # the next layer's GroupNorm statistics ride in this conv's epilogue
        assert ksize == 3 and gn_sums.dtype == torch.int64 and gn_sums.numel() == N * (Nc // 16) * 2
        check(lib.mi_conv3x3_bf16w_io_gnsums(C.byref(d), _p(x), _p(x2), _p(wsh), _p(bias), _p(residual), _p(out), io, _p(gn_sums), _stream()),
              "mi_conv3x3_bf16w_io_gnsums")
    elif io:
        check(lib.mi_conv3x3_bf16w_io(C.byref(d), _p(x), _p(x2), _p(wsh), _p(bias), _p(residual), _p(out), io, _stream()),
              "mi_conv3x3_bf16w_io")
    else:
        check(lib.mi_conv3x3_bf16w(C.byref(d), _p(x), _p(x2), _p(wsh), _p(bias), _p(residual), _p(out), _stream()),
              "mi_conv3x3_bf16w")
    if e0 is not None:
        bm, ck, sk = C.c_int(), C.c_int(), C.c_int()
        lib.mi_conv3x3_bf16w_tile(C.byref(d), io, C.byref(bm), C.byref(ck), C.byref(sk))
        nb = (N * H * W * K * _esz(x) + N * H * W * Nc * (_esz(out) * (2 if accumulate else 1) + _esz(residual))
              + ksize * ksize * K * Nc * 2)
        _probe_close(e0, f"conv3x3_halo_kernel<{bm.value}, {ck.value}, {ksize}, {'true' if sk.value else 'false'}, {io}, {8 if bm.value == 256 or (bm.value == 128 and ck.value == 64) else 4}>",
                     2.0 * N * H * W * Nc * K * ksize * ksize,
                     f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} flip{int(flip)} acc{int(accumulate)} io{io}", nb)
    return (out, y16) if want16 else out


def gn_stats_coef(x, gamma, beta, *, groups=8, eps=1e-5, temb=None):
    """GroupNorm statistics of x only: -> (stats [N,G,2] = mean, rstd; coef [3,N,C] = scale, shift, time bias) for
    conv3x3_gn_mish, which applies GroupNorm + Mish (+ time bias) while it stages its input (ddpm.py:112-120,139-140)."""
    _need_gpu(x)
    N, H, W, Cc = x.shape
    stats = torch.empty((N, groups, 2), device=x.device, dtype=torch.float32)
    coef = torch.empty((3, N, Cc), device=x.device, dtype=torch.float32)
    d = MiGnDesc(N=N, HW=H * W, C=Cc, G=groups, eps=eps, ldx=ld_of(x), ldy=Cc, ldr=0)
    e0 = _probe_open()
    check(load_library().mi_gn_stats_coef(C.byref(d), _p(x), _p(gamma), _p(beta), _p(temb), ld_of(temb) if temb is not None else 0,
                                          _p(stats), _p(coef), _b16(x), _stream()), "mi_gn_stats_coef")
    if e0 is not None:
        _probe_close(e0, f"gn_mish_fwd_kernel<io{_b16(x)}> (statistics only)", 0.0, f"N{N} HW{H * W} C{Cc}", N * H * W * Cc * _esz(x))
    return stats, coef


GSUM_SCALE = float(1 << 20)      # csrc/common.h MI_GSUM_SCALE: the epilogue sums are 64-bit fixed point (integer atomics: order-independent)


def gn_sums_buffer(N, Nc, device):
    """Zeroed [N][Nc / 16][2] buffer for the (sum, sum of squares) a conv's epilogue accumulates (gn_sums=...)."""
    return torch.zeros(N * (Nc // 16) * 2, device=device, dtype=torch.int64)


def gn_sums_encode(sums_f64):
    """float sums [N][Nc / 16][2] -> the fixed-point buffer the kernels read (tests, benchmarks)."""
    return torch.round(sums_f64.double() * GSUM_SCALE).to(torch.int64).contiguous().view(-1)


def gn_sums_decode(buf):
    return buf.double() / GSUM_SCALE


def gn_coef_from_sums(sums, N, HW, gamma, beta, *, groups=8, eps=1e-5, temb=None):
    """-> (stats [N][G][2], coef [3][N][C]) from the (sum, sum of squares) per sample and 16-channel slab that the producing conv's
    epilogue accumulated (conv3x3_bf16w(..., gn_sums=sums)): what gn_stats_coef computes with a pass over the tensor."""
    Cc = gamma.numel()
    stats = torch.empty((N, groups, 2), device=sums.device, dtype=torch.float32)
    coef = torch.empty((3, N, Cc), device=sums.device, dtype=torch.float32)
    e0 = _probe_open()
    check(load_library().mi_gn_coef_from_sums(N, Cc, groups, HW, eps, _p(sums), _p(gamma), _p(beta), _p(temb),
                                              ld_of(temb) if temb is not None else 0, _p(stats), _p(coef), _stream()), "mi_gn_coef_from_sums")
    if e0 is not None:
        _probe_close(e0, "gn_coef_from_sums_kernel", 0.0, f"N{N} C{Cc}", N * Cc * 16.0)
    return stats, coef


def gn_mish_apply_sums(x, sums, gamma, beta, *, groups=8, eps=1e-5, temb=None, residual=None, out_dtype=torch.float32, want16=False):
    """GroupNorm + Mish (+ time bias) (+ residual) as one streaming pass over x (bf16, the output of a conv that ran with gn_sums=sums):
    the statistics come from the conv's epilogue sums, so there is no statistics phase.  -> (y, stats[, y16]) like gn_mish_fwd, or None when
    the library does not take the shape (the caller then runs gn_mish_fwd)."""
    _need_gpu(x)
    if x.dtype != torch.bfloat16:
        return None
    N, H, W, Cc = x.shape
    y16 = None
    y = new_act(N, H, W, Cc, x, out_dtype)
    if want16:
        assert out_dtype == torch.float32
        y16 = new_act(N, H, W, Cc, x, torch.bfloat16)
    stats = torch.empty((N, groups, 2), device=x.device, dtype=torch.float32)
    d = MiGnDesc(N=N, HW=H * W, C=Cc, G=groups, eps=eps, ldx=ld_of(x), ldy=ld_of(y), ldr=ld_of(residual) if residual is not None else 0)
    e0 = _probe_open()
    rc = load_library().mi_gn_mish_apply_sums(C.byref(d), _p(x), _p(sums), _p(gamma), _p(beta), _p(temb), ld_of(temb) if temb is not None else 0,
                                              _p(residual), _p(y), _b16(y), _p(y16), ld_of(y16) if y16 is not None else 0, _p(stats), _stream())
    if rc == 1:
        return None
    check(rc, "mi_gn_mish_apply_sums")
    if e0 is not None:
        _probe_close(e0, f"gn_apply_sums_kernel<io{1 + 2 * _b16(y)}>", 0.0, f"N{N} HW{H * W} C{Cc}",
                     N * H * W * Cc * (_esz(x) + _esz(y) + _esz(residual) + _esz(y16)))
    return (y, stats, y16) if want16 else (y, stats)


@_cached_question
def conv3x3_gn_mish_supported(N, H, W, K, Nc):
    return bool(_query("mi_conv3x3_gn_mish_supported", _conv_desc(N, H, W, K, Nc, 3, ldx2=K)))


@_cached_question
def conv3x3_pw_gn_mish_picked(N, H, W, K, Nc):
    """Does conv3x3_gn_mish route a bf16-stored layer of this shape to the private-weight-stream fused kernel (given wq)?"""
    d = _conv_desc(N, H, W, K, Nc, 3, ldx2=K)
    # Where it pays (measured in the B = 64 sampler, round 4): every 64-channel chunk of K costs the fused kernel one transform block
    # (~1 us that the matrix pipe of that workgroup waits for), the GroupNorm pass it replaces costs ~4 us + its bytes -- the fusion
    # wins up to K = 256 (level 0: -2.3 us per block, 256 channels @16x16: -4 us) and loses on the 512-channel 8x8 layers (+2 us)
    # (round 6, the fused variants on the pinned loop: K = 512 is break-even or slightly ahead -- sampler 994-1 003 -> 1 002-1 004 steps/s)
    return bool(USE_CONV_PW and K <= int(debug_knob("MI_FUSE_GN_MAXK", "512")) and _pick_pw_fused(N, H, W, Nc, d, False))


def _pick_pw_fused(N, H, W, Nc, d, in32):
    """Tile (128 / 64 pixels; 0 = no) the fused GroupNorm + Mish + conv variants of the private-weight-stream kernel would run this
    layer with -- the library's pick, subject to the same minimum grid as the plain conv."""
    pt = _query("mi_conv3x3_pw_x32_gn_mish_tile" if in32 else "mi_conv3x3_pw_gn_mish_tile", d)
    return pt if pt and (N * H * W // pt) * ((Nc + 127) // 128) >= PW_MIN_TILES else 0


def conv3x3_gn_mish(x, coef, wsh, *, K, Nc, bias=None, out_dtype=None, gn=None, wq=None):
    """The fused kernel BASELINE.json names: y = conv3x3(mish(x * scale + shift) + tb) + bias with x the RAW previous conv output
    (fp32 -> fp32 y, or bf16 -> bf16 y), coef from gn_stats_coef -- or coef = None and gn = (sums, gamma, beta, temb, groups, eps):
    the statistics come from the sums the producing conv's epilogue left (conv3x3_bf16w(..., gn_sums=sums)) and are resolved inside
    the kernel.  Returns None when the shape is not supported."""
    _need_gpu(x)
    N, H, W, _ = x.shape
    d = _conv_desc(N, H, W, K, Nc, 3, ldx=ld_of(x), ldx2=ld_of(x))
    lib = load_library()
    ptf = _pick_pw_fused(N, H, W, Nc, d, x.dtype == torch.float32) if (wq is not None and USE_CONV_PW) else 0
    if ptf and x.dtype == torch.bfloat16:
        # the private-weight-stream kernel: the transform runs once per staged element, in place in LDS
        y = new_act(N, H, W, Nc, x, x.dtype if out_dtype is None else out_dtype)
        d.ldy = Nc
        e0 = _probe_open()
        if coef is None and (K // gn[4]) not in (16, 32, 64):
            _, coef = gn_coef_from_sums(gn[0], N, H * W, gn[1], gn[2], groups=gn[4], eps=gn[5], temb=gn[3])
        if coef is None:          # statistics, affine and time bias resolved inside the kernel from the producer's sums
            sums, gamma, beta, temb, groups, eps = gn
            check(lib.mi_conv3x3_pw_gn_mish_sums(C.byref(d), _p(x), _p(sums), _p(gamma), _p(beta), _p(temb),
                                                 ld_of(temb) if temb is not None else 0, groups, eps, _p(wq), _p(bias), _p(y), _b16(y),
                                                 _stream()), "mi_conv3x3_pw_gn_mish_sums")
        else:
            check(lib.mi_conv3x3_pw_gn_mish(C.byref(d), _p(x), _p(coef), _p(wq), _p(bias), _p(y), _b16(y), _stream()), "mi_conv3x3_pw_gn_mish")
        if e0 is not None:
            _probe_close(e0, f"conv_pw_kernel<{'true' if _b16(y) else 'false'}, {3 if coef is None else 2}, 0, {_pw_tile_now(d, 2, False, ptf)}>", 2.0 * N * H * W * Nc * K * 9,
                         f"N{N} {H}x{W} K{K}->{Nc} fused GN+Mish", N * H * W * (K * 2 + Nc * _esz(y)) + 9 * K * Nc * 2)
        return y
    if ptf and x.dtype == torch.float32:
        # fp32-stored activations on the same kernel (round 4): the transform is applied to the fp32 values in registers, between
        # their load and the one rounding to bf16
        y = new_act(N, H, W, Nc, x, x.dtype if out_dtype is None else out_dtype)
        d.ldy = Nc
        e0 = _probe_open()
        if coef is None and (K // gn[4]) not in (16, 32, 64):
            _, coef = gn_coef_from_sums(gn[0], N, H * W, gn[1], gn[2], groups=gn[4], eps=gn[5], temb=gn[3])
        if coef is None:
            sums, gamma, beta, temb, groups, eps = gn
            check(lib.mi_conv3x3_pw_x32_gn_mish_sums(C.byref(d), _p(x), _p(sums), _p(gamma), _p(beta), _p(temb),
                                                     ld_of(temb) if temb is not None else 0, groups, eps, _p(wq), _p(bias), _p(y), _b16(y),
                                                     _stream()), "mi_conv3x3_pw_x32_gn_mish_sums")
        else:
            check(lib.mi_conv3x3_pw_x32_gn_mish(C.byref(d), _p(x), _p(coef), _p(wq), _p(bias), _p(y), _b16(y), _stream()),
                  "mi_conv3x3_pw_x32_gn_mish")
        if e0 is not None:
            _probe_close(e0, f"conv_pw_kernel<{'true' if _b16(y) else 'false'}, {3 if coef is None else 2}, 0, {_pw_tile_now(d, 2, True, ptf)}, true>",
                         2.0 * N * H * W * Nc * K * 9, f"N{N} {H}x{W} K{K}->{Nc} fused GN+Mish, fp32 in",
                         N * H * W * (K * 4 + Nc * _esz(y)) + 9 * K * Nc * 2)
        return y
    if not lib.mi_conv3x3_gn_mish_supported(C.byref(d)):
        return None
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype != x.dtype:
        raise RuntimeError("the fused kernel writes y in x's storage type (fp32 -> fp32 or bf16 -> bf16)")
    y = new_act(N, H, W, Nc, x, out_dtype)
    io = 3 if x.dtype == torch.bfloat16 else 0
    e0 = _probe_open()
    if gn is not None:
        sums, gamma, beta, temb, groups, eps = gn
        check(lib.mi_conv3x3_gn_mish_sums(C.byref(d), _p(x), _p(sums), _p(gamma), _p(beta), _p(temb), ld_of(temb) if temb is not None else 0,
                                          groups, eps, _p(wsh), _p(bias), _p(y), io, _stream()), "mi_conv3x3_gn_mish_sums")
    else:
        check(lib.mi_conv3x3_gn_mish(C.byref(d), _p(x), _p(coef), _p(wsh), _p(bias), _p(y), io, _stream()), "mi_conv3x3_gn_mish")
    if e0 is not None:
        bm, ck = C.c_int(), C.c_int()
        lib.mi_conv3x3_gn_mish_tile(C.byref(d), C.byref(bm), C.byref(ck))
        _probe_close(e0, f"conv3x3_halo_kernel<{bm.value}, {ck.value}, 3, false, {io}, {8 if bm.value == 256 else 4}, true>",
                     2.0 * N * H * W * Nc * K * 9, f"N{N} {H}x{W} K{K}->{Nc} fused GN+Mish",
                     N * H * W * (K * _esz(x) + Nc * _esz(y)) + 9 * K * Nc * 2)
    return y


def pack_weights_tile():
    """Tile edge mi_pack_weights_bf16 counts an entry's tiles in (tile0 = running sum of taps * ceil(ci / T) * ceil(co / T))."""
    return int(load_library().mi_pack_weights_tile())


PACK_ENTRY = [("off", "<i8"), ("taps", "<i4"), ("ci", "<i4"), ("co", "<i4"), ("tile0", "<i4"), ("frag", "<i4"), ("pad", "<i4")]


def pack_table(entries, device):
    """Device table for mi_pack_weights_bf16 from (float offset, taps, ci, co) per conv weight -> (table, nent, total tiles).
    3x3 and 1x1 layers with ci % 64 == 0 and co % 64 == 0 are flagged for the MFMA-fragment-order copies (the operands of
    mi_conv3x3_pw / mi_conv1x1_pw)."""
    import numpy as np
    rec = np.zeros(len(entries), dtype=np.dtype(PACK_ENTRY))
    tile, T = 0, pack_weights_tile()
    for i, (off, taps, ci, co) in enumerate(entries):
        rec[i] = (off, taps, ci, co, tile, int(taps in (1, 9, 16) and ci % 64 == 0 and co % 64 == 0), 0)
        tile += taps * ((ci + T - 1) // T) * ((co + T - 1) // T)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device), len(entries), tile


def pack_weights_bf16(table_dev, nent, total_tiles, master, wd, wf, wdq=None, wfq=None):
    """wdq / wfq: the fragment-order copies (same offsets as the master buffer) of the entries the table flags."""
    e0 = _probe_open()
    check(load_library().mi_pack_weights_bf16(nent, _p(table_dev), total_tiles, _p(master), _p(wd), _p(wf), _p(wdq), _p(wfq), _stream()),
          "mi_pack_weights_bf16")
    if e0 is not None:
        _probe_close(e0, "pack_weights_kernel", 0.0, f"{master.numel()} params", master.numel() * (8.0 if wdq is None else 12.0))


def pack_weights_f32frag(table_dev, nent, total_tiles, master, wdq32, wfq32):
    """fp32 fragment-order copies (forward / data-gradient operand of mi_conv3x3_pw_f32) of the entries pack_table flags."""
    e0 = _probe_open()
    check(load_library().mi_pack_weights_f32frag(nent, _p(table_dev), total_tiles, _p(master), _p(wdq32), _p(wfq32), _stream()),
          "mi_pack_weights_f32frag")
    if e0 is not None:
        _probe_close(e0, "pack_f32frag_kernel", 0.0, f"{master.numel()} params", master.numel() * 12.0)


def conv3x3_f32(x, wq32, *, K, Nc, flip, x2=None, bias=None, residual=None, out=None, accumulate=False):
    """3x3/s1/p1 conv (flip=False) or its data gradient (flip=True) in exact-fp32 mode through the private-weight-stream kernel on
    v_mfma_f32_32x32x2_f32 (mi_conv3x3_pw_f32).  wq32: the layer's slice of the fp32 fragment-order copy.  None: not supported."""
    _need_gpu(x)
    if x.dtype != torch.float32 or (x2 is not None and x2.dtype != torch.float32) or not USE_CONV_PW:
        return None
    N, H, W, K1 = x.shape
    if x2 is None:
        K1 = K
    d = _conv_desc(N, H, W, K, Nc, 3, transposed=flip, mode=MODE_FP32, K1=K1, ldx=ld_of(x), ldx2=_ldn(x2), ldr=_ldn(residual), accumulate=accumulate)
    pt = _query("mi_conv3x3_pw_f32_tile", d)
    if not pt:
        return None
    if out is None:
        assert not accumulate
        out = new_act(N, H, W, Nc, x, torch.float32)
    d.ldy = ld_of(out)
    if d.ldy % 8:
        return None
    e0 = _probe_open()
    check(load_library().mi_conv3x3_pw_f32(C.byref(d), _p(x), _p(x2), _p(wq32), _p(bias), _p(residual), _p(out), _stream()), "mi_conv3x3_pw_f32")
    if e0 is not None:
        nb = (N * H * W * K * 4 + N * H * W * Nc * (4 * (2 if accumulate else 1) + _esz(residual)) + 9 * K * Nc * 4)
        _probe_close(e0, f"conv_pw_kernel<false, 0, 0, {pt}, false, true>", 2.0 * N * H * W * Nc * K * 9,
                     f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} fp32 flip{int(flip)} acc{int(accumulate)}", nb)
    return out


def conv1x1_f32(x, wq32, *, K, Nc, flip, x2=None, bias=None, residual=None, out=None, accumulate=False):
    """1x1 conv (flip=False) or its data gradient (flip=True) in exact-fp32 mode through the streaming kernel (mi_conv1x1_pw_f32).
    None: not supported."""
    _need_gpu(x)
    if x.dtype != torch.float32 or (x2 is not None and x2.dtype != torch.float32) or not USE_CONV_PW:
        return None
    N, H, W, K1 = x.shape
    if x2 is None:
        K1 = K
    d = _conv_desc(N, H, W, K, Nc, 1, transposed=flip, mode=MODE_FP32, K1=K1, ldx=ld_of(x), ldx2=_ldn(x2), ldr=_ldn(residual), accumulate=accumulate)
    if not _query("mi_conv1x1_pw_f32_supported", d):
        return None
    if out is None:
        assert not accumulate
        out = new_act(N, H, W, Nc, x, torch.float32)
    d.ldy = ld_of(out)
    if d.ldy % 8 or (residual is not None and d.ldr % 4):
        return None
    e0 = _probe_open()
    check(load_library().mi_conv1x1_pw_f32(C.byref(d), _p(x), _p(x2), _p(wq32), _p(bias), _p(residual), _p(out), _stream()), "mi_conv1x1_pw_f32")
    if e0 is not None:
        nb = (N * H * W * K * 4 + N * H * W * Nc * (4 * (2 if accumulate else 1) + _esz(residual)) + K * Nc * 4)
        px = 64 if (N * H * W // 128) * ((Nc + 127) // 128) < 256 else 128
        _probe_close(e0, f"conv1x1_pw_kernel<false, false, {px}, true>", 2.0 * N * H * W * Nc * K,
                     f"N{N} {H}x{W} K{K}{'(2src)' if x2 is not None else ''}->{Nc} fp32 flip{int(flip)} acc{int(accumulate)}", nb)
    return out


@_cached_question
def small_cin_supported(ks, Cin, Cout, wgrad=False):
    """The 3-channel-input kernels (mi_conv_small_cin_*): which (kernel size, Cin, Cout) they take."""
    if ks not in (1, 3) or not 1 <= Cin <= 4:
        return False
    if wgrad:
        return Cout in (64, 128, 256) and 3 * ks * ks * Cin * (Cout // 4) * 16 <= 48 * 1024
    return Cout >= 4 and Cout % 4 == 0 and Cout <= 1024 and 256 % (Cout // 4) == 0


@_cached_question
def small_cin_bf16_supported(ks, N, H, W, Cin, Cout, ldx):
    """The first Block's conv (Cin <= 4) can write its output as bf16 AND its weight gradient can read a bf16 dy (round 4)."""
    return bool(load_library().mi_conv_small_cin_bf16_supported(ks, N, H, W, Cin, Cout, ldx))


def conv_small_cin_fwd(x, w, bias, Cout, ks, out_dtype=torch.float32):
    """Conv2d(Cin<=4, Cout, ks, padding=ks//2) on an NHWC image tensor (first convs of the UNet); out_dtype bf16: the output rounded
    once on the way out (small_cin_bf16_supported)."""
    _need_gpu(x)
    N, H, W, Cin = x.shape
    y = (torch.empty((N, H, W, Cout), device=x.device, dtype=torch.bfloat16) if out_dtype == torch.bfloat16 else new_act(N, H, W, Cout, x))
    check(load_library().mi_conv_small_cin_fwd_io(ks, N, H, W, Cin, Cout, _p(x), ld_of(x), _p(w), _p(bias), _p(y), ld_of(y), _b16(y), _stream()),
          "mi_conv_small_cin_fwd")
    return y


def conv1x1_small_cout_bwd(x, dy, w, dW, dx, accumulate=False):
    """Backward of the C -> Cs (<= 4) 1x1 conv in one pass over (x, dy): dW[C][Cs] += x^T dy and dx (+)= dy w^T (what conv1x1_small_cout op 2 and
    op 1 compute in two launches; bitwise the same)."""
    _need_gpu(x)
    N, H, W, Cc = x.shape
    Cs = dy.shape[3]
    lib = load_library()
    need = lib.mi_conv_small_wgrad_workspace(4 * Cc)
    ws = _workspace(x.device, need)
    check(lib.mi_conv1x1_small_cout_bwd(N * H * W, Cc, Cs, _p(x), ld_of(x), _b16(x), _p(dy), ld_of(dy), _p(w), _p(dW), _p(dx), ld_of(dx), _b16(dx),
                                        int(accumulate), _p(ws), need, _stream()), "mi_conv1x1_small_cout_bwd")


@_cached_question
def small_cout_gn_supported(C, Cs, G):
    return bool(load_library().mi_conv1x1_small_cout_gn_supported(C, Cs, G))


def conv1x1_small_cout_gn(x, sums, gamma, beta, w, bias, Cs, groups=8, eps=1e-5):
    """Inference, final_conv: y = conv1x1(mish(groupnorm(x))) + bias with x the Block conv's bf16 output and its GroupNorm statistics taken from
    the sums that conv's epilogue left (conv3x3_bf16w(..., gn_sums=sums)) -- one launch, the normalised tensor is never written."""
    _need_gpu(x)
    assert x.dtype == torch.bfloat16 and sums.dtype == torch.int64
    N, H, W, Cc = x.shape
    y = torch.empty((N, H, W, 4), device=x.device, dtype=torch.float32)       # padded 4-channel pixels; the kernel writes the padding (zero) too
    e0 = _probe_open()
    check(load_library().mi_conv1x1_small_cout_gn_fwd(N * H * W, H * W, Cc, Cs, _p(x), ld_of(x), _p(sums), _p(gamma), _p(beta), groups, eps,
                                                      _p(w), _p(bias), _p(y), ld_of(y), _stream()), "mi_conv1x1_small_cout_gn_fwd")
    if e0 is not None:
        _probe_close(e0, f"small_cout_fwd_gn_kernel<{Cc // 32}>", 2.0 * N * H * W * Cc * Cs, f"M{N * H * W} C{Cc}->{Cs} GN+Mish in the load",
                     N * H * W * (Cc * 2 + 16))
    return y[..., :Cs]


@_cached_question
def small_cin_dual_supported(N, H, W, Cin, Cout, ldx):
    return bool(load_library().mi_conv_small_cin_fwd_dual_supported(N, H, W, Cin, Cout, ldx))


def conv_small_cin_fwd_dual(x, w3, bias3, w1, bias1, Cout, out_dtype=torch.float32, zero=None, gather=None):
    """The first ResnetBlock's block1 conv (3x3) and its res_conv (1x1) on the same image in one launch -> (y3 in out_dtype, y1 fp32).
    This is a forward's first launch; it can do the forward's chores whose consumers come later -- zero: an int64 tensor it clears (the pool of
    GroupNorm sums); gather = (table [T, R], idx int64 [B], out [B, R]): out[b] = table[idx[b]] (the sampler's time-bias rows)."""
    _need_gpu(x)
    N, H, W, Cin = x.shape
    y3 = (torch.empty((N, H, W, Cout), device=x.device, dtype=torch.bfloat16) if out_dtype == torch.bfloat16 else new_act(N, H, W, Cout, x))
    y1 = new_act(N, H, W, Cout, x)
    e0 = _probe_open()
    if zero is not None or gather is not None:
        assert zero is None or (zero.dtype == torch.int64 and zero.is_contiguous())
        gt, gi, go = gather if gather is not None else (None, None, None)
        assert gather is None or (gt.is_contiguous() and go.is_contiguous() and gi.dtype == torch.int64 and go.shape == (gi.shape[0], gt.shape[1]))
        check(load_library().mi_conv_small_cin_fwd_dual_chores(N, H, W, Cin, Cout, _p(x), ld_of(x), _p(w3), _p(bias3), _p(y3), ld_of(y3), _b16(y3),
                                                             _p(w1), _p(bias1), _p(y1), ld_of(y1), _p(zero), zero.numel() * 8 if zero is not None else 0,
                                                             _p(gt), _p(gi), _p(go), gt.shape[1] if gather is not None else 0,
                                                             gi.shape[0] if gather is not None else 0, _stream()),
              "mi_conv_small_cin_fwd_dual_chores")
    else:
        check(load_library().mi_conv_small_cin_fwd_dual(N, H, W, Cin, Cout, _p(x), ld_of(x), _p(w3), _p(bias3), _p(y3), ld_of(y3), _b16(y3),
                                                        _p(w1), _p(bias1), _p(y1), ld_of(y1), _stream()), "mi_conv_small_cin_fwd_dual")
    if e0 is not None:
        _probe_close(e0, f"small_cin3x3_fwd_tiled_kernel<{Cin}, {'true' if _b16(y3) else 'false'}, true>", 2.0 * N * H * W * Cout * Cin * 10,
                     f"N{N} {H}x{W} K{Cin}->{Cout} 3x3 + res_conv", N * H * W * (16 + Cout * (_esz(y3) + 4)))
    return y3, y1


def conv_small_cin_wgrad(x, dy, dW, ks):
    N, H, W, Cin = x.shape
    lib = load_library()
    need = lib.mi_conv_small_wgrad_workspace(ks * ks * Cin * dy.shape[3])
    ws = _workspace(x.device, need)
    check(lib.mi_conv_small_cin_wgrad_io(ks, N, H, W, Cin, dy.shape[3], _p(x), ld_of(x), _p(dy), ld_of(dy), _b16(dy), _p(dW), _p(ws), need,
                                         _stream()), "mi_conv_small_cin_wgrad")


@_cached_question
def small_cout_supported(op, C, Cs):
    """Conv2d(C, Cs<=4, 1) kernels (mi_conv1x1_small_cout): op 0 forward, 1 dgrad, 2 wgrad."""
    if not 1 <= Cs <= 4 or C not in (32, 64, 128, 256):
        return False
    return C <= 128 if op == 0 else (C >= 64 if op == 2 else True)


def conv1x1_small_cout(op, a, w, *, b=None, bias=None, out=None, Cs=None, accumulate=False):
    """op 0: y[.,Cs] = x w + bias; op 1: dx[.,C] (+)= dy w^T; op 2: dW[C][Cs] += x^T dy.  w: [C][Cs]."""
    _need_gpu(a)
    N, H, W = a.shape[:3]
    M = N * H * W
    if op == 0:
        C, Cs = a.shape[3], Cs
        if out is None:
            buf = torch.empty((N, H, W, (Cs + 3) // 4 * 4), device=a.device, dtype=torch.float32)      # (the kernel writes the padding channels: zeros)
            out = buf[..., :Cs]
    elif op == 1:
        Cs = a.shape[3]; C = out.shape[3]
    else:
        C, Cs = a.shape[3], b.shape[3]
    lib = load_library()
    need = lib.mi_conv_small_wgrad_workspace(4 * C) if op == 2 else 0
    ws = _workspace(a.device, need) if op == 2 else None
    wide16 = _b16(out) if op == 1 else _b16(a)       # the C-channel tensor: x (op 0 / 2) or dx (op 1)
    check(lib.mi_conv1x1_small_cout_io(op, M, C, Cs, _p(a), ld_of(a), _p(b), ld_of(b) if b is not None else 0, _p(w),
                                       _p(bias), _p(out), ld_of(out) if out.dim() == 4 else Cs, int(accumulate), wide16, _p(ws), need, _stream()),
          "mi_conv1x1_small_cout")
    return out


def conv_wgrad(P, Q, dW, *, kh, kw, stride, pad, gather_i, Ci, Cj, grid_g, grid_d, mode, P2=None, dbias=None, ordered=False):
    """dW[tap][i][j] += sum P*Q (see MiWgradDesc).  dW: flat fp32 buffer of kh*kw*Ci*Cj.
    dbias (optional): dbias[j] += sum over pixels of Q -- fused when the fast kernel runs, else a colsum pass.
    ordered: the generic kernel in slab mode (mi_conv_wgrad_slabs) and the ordered column sum -- partial sums are stored and added
    in a fixed order, no atomics: two runs give the same bits (fp32 operands)."""
    _need_gpu(P)
    N = P.shape[0]
    d = _wgrad_desc(N, grid_g, grid_d, Ci, Cj, (kh, kw), stride, pad, gather_i, mode, ld_of(P), ld_of(Q),
                    I1=P.shape[3] if P2 is not None else Ci, ldp2=_ldn(P2))
    lib = load_library()
    if ordered:
        if _b16(P) or _b16(Q):
            raise RuntimeError("conv_wgrad(ordered=True) takes fp32 operands")
        ws = _workspace(P.device, lib.mi_conv_wgrad_slabs_workspace(C.byref(d)))
        check(lib.mi_conv_wgrad_slabs(C.byref(d), _p(P), _p(P2), _p(Q), _p(dW), _p(ws), ws.numel() * 4, _stream()), "mi_conv_wgrad_slabs")
        if dbias is not None:
            colsum(Q, dbias, ordered=True)
        return
    fast = bool(lib.mi_conv3x3_wgrad_supported(C.byref(d)))
    use_tr = bool(USE_WGRAD_TR and dbias is None and kh == 3 and _b16(P) and _b16(Q) and (P2 is None or _b16(P2))
                  and _query("mi_conv3x3_wgrad_tr_supported", d))
    if not fast and not use_tr and (_b16(P) or _b16(Q)):
        raise RuntimeError("bf16-stored operands need the fast wgrad kernel (caller must check wgrad_supported)")
    flops = 2.0 * N * grid_d[0] * grid_d[1] * Ci * Cj * kh * kw
    nb_in = N * grid_g[0] * grid_g[1] * Ci * _esz(P) + N * grid_d[0] * grid_d[1] * Cj * _esz(Q)
    desc = f"N{N} {grid_d[0]}x{grid_d[1]} Ci{Ci}{'(2src)' if P2 is not None else ''} Cj{Cj} k{kh} s{stride} g{int(gather_i)}"
    if use_tr:
        # both operands bf16-stored: LDS-DMA + transposing-read kernel, all nine taps per workgroup
        need = lib.mi_conv3x3_wgrad_tr_workspace(C.byref(d))
        ws = _workspace(P.device, need)

        def go_tr():
            check(lib.mi_conv3x3_wgrad_tr(C.byref(d), _p(P), _p(P2), _p(Q), _p(dW), _p(ws), ws.numel() * 4, _stream()), "mi_conv3x3_wgrad_tr")
        if PROBE is None:
            go_tr()
        else:
            sp = lib.mi_conv3x3_wgrad_tr_splits(C.byref(d))
            part = 9.0 * 64 * 128 * 4 * sp * (Ci // 64) * ((Cj + 127) // 128)
            try:
                lib.mi_debug_wgrad_tr_phase(1)
                e0 = _probe_open(); go_tr(); _probe_close(e0, "wgrad_tr_kernel", flops, desc, nb_in + part)
                lib.mi_debug_wgrad_tr_phase(2)
                e0 = _probe_open(); go_tr()
                _probe_close(e0, "wgrad_tr_reduce_kernel", 0.0, desc + f" splits{sp}", part + 9.0 * Ci * Cj * 8)
            finally:
                lib.mi_debug_wgrad_tr_phase(0)
        return
    if fast:
        need = lib.mi_conv3x3_wgrad_workspace(C.byref(d))
        ws = _workspace(P.device, need)
        io = _b16(P) | (_b16(Q) << 1)

        def go():
            if io:
                check(lib.mi_conv3x3_wgrad_io(C.byref(d), _p(P), _p(P2), _p(Q), _p(dW), _p(dbias), _p(ws), ws.numel() * 4, io, _stream()),
                      "mi_conv3x3_wgrad_io")
            else:
                check(lib.mi_conv3x3_wgrad_bias(C.byref(d), _p(P), _p(P2), _p(Q), _p(dW), _p(dbias), _p(ws), ws.numel() * 4, _stream()),
                      "mi_conv3x3_wgrad_bias")
        if PROBE is None:
            go()
        else:                         # time the contraction kernel and the partial-tile reduce under separate events
            nj, sp = C.c_int(), C.c_int()
            lib.mi_conv3x3_wgrad_tile(C.byref(d), C.byref(nj), C.byref(sp))
            sym = f"wgrad3x3_kernel<{nj.value}, {kh}, {io}>"
            part = kh * kw * Ci * Cj * 4.0 * sp.value
            if sp.value > 1:
                try:
                    lib.mi_debug_wgrad3x3_phase(1)
                    e0 = _probe_open(); go(); _probe_close(e0, sym, flops, desc, nb_in + part)
                    lib.mi_debug_wgrad3x3_phase(2)
                    e0 = _probe_open(); go()
                    _probe_close(e0, f"wgrad_reduce_kernel<{16 if sp.value >= 128 else 4}>", 0.0, desc + f" splits{sp.value}", part + kh * kw * Ci * Cj * 8.0)
                finally:
                    lib.mi_debug_wgrad3x3_phase(0)
            else:
                e0 = _probe_open(); go(); _probe_close(e0, sym, flops, desc, nb_in + kh * kw * Ci * Cj * 8.0)
    else:
        e0 = _probe_open()
        check(lib.mi_conv_wgrad(C.byref(d), _p(P), _p(P2), _p(Q), _p(dW), _stream()), "mi_conv_wgrad")
        if e0 is not None:
            _probe_close(e0, f"wgrad_kernel<{mode}>", flops, desc, nb_in + kh * kw * Ci * Cj * 8.0)
        if dbias is not None:
            colsum(Q, dbias)


def conv_s2_wgrad_f32(P, Q, dW, *, k, Ci, Cj, gather_i, grid_g, grid_d):
    """Exact-fp32 mode: the weight gradient of Downsample (3x3 / stride 2, gather_i: P is the big tensor) or Upsample (ConvTranspose 4x4 /
    stride 2: Q is) as k x k gathered problems of the fp32 1x1 weight-gradient kernel (mi_conv_s2_wgrad_f32).  dW [k][k][Ci][Cj] +=.
    Returns True when the library took the layer, False when the caller has to use conv_wgrad."""
    if P.dtype != torch.float32 or Q.dtype != torch.float32:
        return False
    _need_gpu(P)
    N = P.shape[0]
    d = _wgrad_desc(N, grid_g, grid_d, Ci, Cj, k, 2, 1, gather_i, MODE_FP32, ld_of(P), ld_of(Q))
    if not _query("mi_conv_s2_wgrad_f32_supported", d):
        return False
    lib = load_library()
    need = lib.mi_conv_s2_wgrad_f32_workspace(C.byref(d))
    ws = _workspace(P.device, need)
    e0 = _probe_open()
    check(lib.mi_conv_s2_wgrad_f32(C.byref(d), _p(P), _p(Q), _p(dW), _p(ws), ws.numel() * 4, _stream()), "mi_conv_s2_wgrad_f32")
    if e0 is not None:
        _probe_close(e0, "wgrad1x1_f32_kernel[s2 taps]", 2.0 * N * grid_d[0] * grid_d[1] * Ci * Cj * k * k, f"N{N} {grid_d[0]}x{grid_d[1]} Ci{Ci} Cj{Cj} k{k}",
                     N * (grid_g[0] * grid_g[1] * (Ci if gather_i else Cj) + grid_d[0] * grid_d[1] * (Cj if gather_i else Ci)) * 4.0)
    return True


@_cached_question
def s2_wgrad_supported(N, k, Ci, Cj, transposed, big, small, mode):
    """Can the stride-2 LDS-DMA weight-gradient kernel take this Downsample (3x3 conv) / Upsample (4x4 transposed conv) layer
    (dense bf16 operands)?  big / small: the (H, W) of the 2x-resolution tensor and of the other one."""
    return bool(USE_WGRAD_TR and _query("mi_conv_s2_wgrad_tr_supported", _wgrad_desc(N, big, small, Ci, Cj, k, 2, 1, not transposed, mode, Ci, Cj)))


@_cached_question
def conv_gt_supported(N, IH, IW, K, Nc, k, transposed):
    """Does the tap-gather kernel take the Downsample (k = 3) / Upsample (k = 4, transposed) forward conv on a dense bf16 input?"""
    out_hw = (2 * IH, 2 * IW) if transposed else ((IH + 2 - k) // 2 + 1, (IW + 2 - k) // 2 + 1)
    return bool(USE_CONV_GT and Nc % 8 == 0 and _query("mi_conv_gt_supported", _conv_desc(N, IH, IW, K, Nc, k, out_hw=out_hw, stride=2, pad=1, transposed=transposed)))


class WgradQueue:
    """Deferred weight gradients of the Block convs (3x3) and of the 1x1 convs.  The queue holds the operands it was handed until
    their launch (items3 / items1 / items2): a caller need not keep them alive, but must not write into them before the flush.
    Backward pushes (X, dY, dW) here instead of launching one full-chip kernel per layer; every `group` layers of a kind go out as ONE launch (mi_conv3x3_wgrad_tr_batch /
    mi_conv1x1_wgrad_tr_batch), each layer on its share of the CUs (see include/mi_ddpm.h: an eighth of the partial-tile traffic,
    an eighth of the launches).  Layers the LDS-DMA kernels cannot take run at once through conv_wgrad.  `pushed` numbers the deferred
    layers (1, 2, ...); `flushed` = the largest n such that layers 1..n have ALL been issued (the two kinds flush independently, so a
    count of issued layers would not say that); `on_flush()` is called after every flush.
    Kind 4 (round 4): reductions that leave one partial row per workgroup (channel LayerNorm's dg / db) push (rows, dst) pairs; ONE
    mi_rowsum_batch launch adds all of them (at the final flush, or right away when a caller flushes kind 4: data parallelism).
    store: the launches WRITE dW (MI_WGRAD_STORE) -- for a gradient buffer whose conv weights were left unfilled; a layer that falls
    back to conv_wgrad (which can only add) and was pushed with prefill=True has its dW zero-filled first."""

    def __init__(self, group: int = 8, on_flush=None, group_s2=None, store=False):
        self.group, self.on_flush = max(1, min(8, int(group))), on_flush
        self.flags = WGRAD_STORE if store else 0
        self.group_s2 = self.group if group_s2 is None else max(1, min(8, int(group_s2)))    # stride-2 layers per launch
        self.items3, self.items1, self.items2, self.items4 = [], [], [], []
        self.pushed = 0
        self._seq3, self._seq1, self._seq2, self._seq4 = [], [], [], []        # sequence numbers of the queued layers, per kind
        self._arena_top = 0                                    # partial rows of this backward pass (see rows_buffer)

    @property
    def flushed(self) -> int:
        pending = self._seq3[:1] + self._seq1[:1] + self._seq2[:1] + self._seq4[:1]
        return min(pending) - 1 if pending else self.pushed

    def _desc(self, P, Q, k, Ci, Cj, hw, mode, P2):
        return _wgrad_desc(P.shape[0], hw, hw, Ci, Cj, k, 1, k // 2, True, mode, ld_of(P), ld_of(Q),
                           I1=P.shape[3] if P2 is not None else Ci, ldp2=_ldn(P2))

    def push(self, P, Q, dW, *, Ci, Cj, hw, mode, P2=None, prefill=False):
        """3x3 / stride 1 / pad 1.  prefill: dW holds no zeros yet (store mode) -- filled here if the layer takes the fallback"""
        d = self._desc(P, Q, 3, Ci, Cj, hw, mode, P2)
        same = (lambda dt: P.dtype == dt and Q.dtype == dt and (P2 is None or P2.dtype == dt))      # noqa: E731
        ok = (USE_WGRAD_TR and self.group > 1 and (same(torch.bfloat16) if mode == MODE_BF16 else same(torch.float32))
              and _query("mi_conv3x3_wgrad_tr_supported", d))      # (mode 0: the exact-fp32 instantiation, fp32 operands)
        if not ok:
            if prefill:
                dW.zero_()
            conv_wgrad(P, Q, dW, kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=Ci, Cj=Cj, grid_g=hw, grid_d=hw, mode=mode, P2=P2)
            return
        self.items3.append((d, P, P2, Q, dW))
        self.pushed += 1
        self._seq3.append(self.pushed)
        if len(self.items3) >= self.group:
            self.flush(kinds=(3,))

    def push1x1(self, P, Q, dW, *, Ci, Cj, hw, mode, P2=None, dbias=None, prefill=False):
        """1x1; dbias (optional) += column sums of Q; prefill: as in push"""
        d = self._desc(P, Q, 1, Ci, Cj, hw, mode, P2)
        q32 = int(Q.dtype == torch.float32)
        if mode == MODE_FP32:       # exact-fp32 instantiation (round 4): fp32 X and dY
            dt_ok = P.dtype == torch.float32 and (P2 is None or P2.dtype == torch.float32) and q32
        else:
            dt_ok = _b16(P) and (P2 is None or _b16(P2))
        ok = (USE_WGRAD_TR and self.group > 1 and dt_ok and (dbias is None or q32)
              and _query("mi_conv1x1_wgrad_tr_supported", d, q32))
        if not ok:
            if prefill:
                dW.zero_()
            conv_wgrad(P, Q, dW, kh=1, kw=1, stride=1, pad=0, gather_i=True, Ci=Ci, Cj=Cj, grid_g=hw, grid_d=hw, mode=mode, P2=P2, dbias=dbias)
            return
        self.items1.append((d, P, P2, Q, dW, dbias, q32))
        self.pushed += 1
        self._seq1.append(self.pushed)
        if len(self.items1) >= self.group:
            self.flush(kinds=(1,))

    def push_s2(self, P, Q, dW, *, k, Ci, Cj, gather_i, grid_g, grid_d, mode):
        """Downsample (3x3 / stride 2 / pad 1 conv: gather_i, P = X on the 2x grid) and Upsample (4x4 / stride 2 / pad 1 transposed
        conv: not gather_i, Q = dY on the 2x grid) weight gradients; both operands bf16.  Returns False when the LDS-DMA kernel
        cannot take the layer (the caller then runs conv_wgrad)."""
        d = _wgrad_desc(P.shape[0], grid_g, grid_d, Ci, Cj, k, 2, 1, gather_i, mode, ld_of(P), ld_of(Q))
        if not (USE_WGRAD_TR and _b16(P) and _b16(Q) and _query("mi_conv_s2_wgrad_tr_supported", d)):
            return False
        self.items2.append((d, P, None, Q, dW))
        self.pushed += 1
        self._seq2.append(self.pushed)
        if len(self.items2) >= self.group_s2:
            self.flush(kinds=(2,))
        return True

    def rows_buffer(self, device, nfloats):
        """nfloats of the persistent partial-row arena (static address: capturable); valid until the next backward pass"""
        n = (int(nfloats) + 63) // 64 * 64
        arena = _rows_arena(device, (self._arena_top + n) * 4)
        out = arena[self._arena_top:self._arena_top + n]
        self._arena_top += n
        return out

    def push_rowsum(self, src, rows, cols, ld, dst):
        """dst[c] += sum_r src[r * ld + c] (deferred)"""
        self.items4.append((src, int(rows), int(cols), int(ld), dst))
        self.pushed += 1
        self._seq4.append(self.pushed)

    def flush(self, kinds=(3, 1, 2, 4)):
        lib = load_library()
        if 4 in kinds and self.items4:
            items, self.items4, self._seq4 = self.items4, [], []
            _need_gpu(items[0][0])
            for i0 in range(0, len(items), ROWSUM_MAX):
                chunk = items[i0:i0 + ROWSUM_MAX]
                arr4 = (MiRowSum * len(chunk))(*[MiRowSum(src=it[0].data_ptr(), dst=it[4].data_ptr(), rows=it[1], cols=it[2], ld=it[3], pad_=0)
                                                 for it in chunk])
                e0 = _probe_open()
                check(lib.mi_rowsum_batch(len(chunk), arr4, _stream()), "mi_rowsum_batch")
                if e0 is not None:
                    _probe_close(e0, "rowsum_batch_kernel", 0.0, f"{len(chunk)} items", sum(it[1] * it[2] * 4.0 for it in chunk))
        arr = lambda items, k: (C.c_void_p * len(items))(*[(it[k].data_ptr() if it[k] is not None else 0) for it in items])   # noqa: E731
        if 3 in kinds and self.items3:
            items, self.items3, self._seq3 = self.items3, [], []
            _need_gpu(items[0][1])
            n = len(items)
            descs = (MiWgradDesc * n)(*[it[0] for it in items])
            need = lib.mi_conv3x3_wgrad_tr_batch_workspace(n, descs)
            ws = _workspace(items[0][1].device, need)

            def go():
                check(lib.mi_conv3x3_wgrad_tr_batch_ex(n, descs, arr(items, 1), arr(items, 2), arr(items, 3), arr(items, 4), _p(ws), ws.numel() * 4,
                                                       _stream(), self.flags), "mi_conv3x3_wgrad_tr_batch_ex")
            flops = sum(2.0 * it[0].N * it[0].DH * it[0].DW * it[0].Ci * it[0].Cj * 9 for it in items)
            f32 = items[0][0].mode == MODE_FP32
            nb = sum(it[0].N * it[0].DH * it[0].DW * (it[0].Ci + it[0].Cj) * (4.0 if f32 else 2.0) for it in items)
            self._run(go, lib.mi_debug_wgrad_tr_phase, "wgrad_tr32" if f32 else "wgrad_tr", n, flops, nb, need)
        if 1 in kinds and self.items1:
            items, self.items1, self._seq1 = self.items1, [], []
            _need_gpu(items[0][1])
            n = len(items)
            descs = (MiWgradDesc * n)(*[it[0] for it in items])
            q32 = (C.c_int * n)(*[it[6] for it in items])
            need = lib.mi_conv1x1_wgrad_tr_batch_workspace(n, descs, q32)
            ws = _workspace(items[0][1].device, need)

            def go1():
                check(lib.mi_conv1x1_wgrad_tr_batch_ex(n, descs, q32, arr(items, 1), arr(items, 2), arr(items, 3), arr(items, 4), arr(items, 5),
                                                       _p(ws), ws.numel() * 4, _stream(), self.flags), "mi_conv1x1_wgrad_tr_batch_ex")
            flops = sum(2.0 * it[0].N * it[0].DH * it[0].DW * it[0].Ci * it[0].Cj for it in items)
            f32 = items[0][0].mode == MODE_FP32
            nb = sum(it[0].N * it[0].DH * it[0].DW * (it[0].Ci * (4.0 if f32 else 2.0) + it[0].Cj * (4.0 if it[6] else 2.0)) for it in items)
            self._run(go1, lib.mi_debug_wgrad1x1_tr_phase, "wgrad1x1_f32" if f32 else "wgrad1x1_tr", n, flops, nb, need)
        if 2 in kinds and self.items2:
            items, self.items2, self._seq2 = self.items2, [], []
            _need_gpu(items[0][1])
            n = len(items)
            descs = (MiWgradDesc * n)(*[it[0] for it in items])
            need = lib.mi_conv_s2_wgrad_tr_batch_workspace(n, descs)
            ws = _workspace(items[0][1].device, need)

            def go2():
                check(lib.mi_conv_s2_wgrad_tr_batch_ex(n, descs, arr(items, 1), arr(items, 3), arr(items, 4), _p(ws), ws.numel() * 4, _stream(),
                                                       self.flags), "mi_conv_s2_wgrad_tr_batch_ex")
            flops = sum(2.0 * it[0].N * it[0].DH * it[0].DW * it[0].Ci * it[0].Cj * it[0].KH * it[0].KW for it in items)
            nb = sum(it[0].N * it[0].DH * it[0].DW * 2.0 * ((4 if it[0].gather_i else 1) * it[0].Ci + (1 if it[0].gather_i else 4) * it[0].Cj)
                     for it in items)
            self._run(go2, lib.mi_debug_wgrad_s2_tr_phase, "wgrad_s2_tr", n, flops, nb, need)
        if self.on_flush is not None:
            self.on_flush()

    @staticmethod
    def _run(go, phase, name, n, flops, nb, need):
        if PROBE is None:
            go()
            return
        try:                                   # contraction and partial-tile reduce under separate events
            phase(1)
            e0 = _probe_open(); go(); _probe_close(e0, name + "_kernel", flops, f"{n} layers", nb + need)
            phase(2)
            e0 = _probe_open(); go(); _probe_close(e0, name.replace("tr32", "tr").replace("1x1_f32", "1x1_tr") + "_reduce_kernel", 0.0, f"{n} layers", float(need))
        finally:
            phase(0)


_WS = {}
_WS_RETIRED = []      # outgrown workspaces stay allocated: a captured hipGraph may still write its partial tiles there
_ROWS = {}


def _rows_arena(device, nbytes):
    """Persistent per-device buffer of the partial rows a backward pass defers (WgradQueue.rows_buffer); grows like _workspace."""
    cur = _ROWS.get(device)
    if cur is None or cur.numel() * 4 < nbytes:
        if cur is not None:
            _WS_RETIRED.append(cur)
        cur = torch.empty((max(int(nbytes) * 2, 16 << 20) + 3) // 4, device=device, dtype=torch.float32)
        _ROWS[device] = cur
    return cur


def zero_ranges(table, n, base):
    """base[off : off + cnt] = 0 for the n (off, cnt) int64 pairs of the device tensor `table`: one kernel launch"""
    e0 = _probe_open()
    check(load_library().mi_zero_ranges(_p(table), int(n), _p(base), _stream()), "mi_zero_ranges")
    if e0 is not None:
        _probe_close(e0, "zero_ranges_kernel", 0.0, f"{n} ranges", 0.0)


def _workspace(device, nbytes):
    """Persistent per-device scratch.  The address a launch saw stays valid for the life of the process (captured hipGraphs
    keep referencing it): when a later call needs more, a larger buffer is added and the old one is retired, never freed."""
    cur = _WS.get(device)
    if cur is None or cur.numel() * 4 < nbytes:
        if cur is not None:
            _WS_RETIRED.append(cur)
        cur = torch.empty((max(int(nbytes), 64 << 20) + 3) // 4, device=device, dtype=torch.float32)
        _WS[device] = cur
    return cur


def _rows(x):
    return x.shape[0] * x.shape[1] * x.shape[2] if x.dim() == 4 else x.shape[0]


def colsum(x, out, defer=None, ordered=False):
    """out[c] += sum over pixels of x[..., c]; defer (a WgradQueue): as partial rows, added by the queue's batched row sum;
    ordered: partial rows stored and added in a fixed order (mi_colsum_ordered: no atomics, two runs give the same bits)"""
    Cc = x.shape[-1]
    M = _rows(x)
    if ordered:
        _need_gpu(x)
        if x.dtype != torch.float32:
            raise RuntimeError("colsum(ordered=True) takes an fp32 tensor")
        lib = load_library()
        ws = _workspace(x.device, lib.mi_colsum_ordered_workspace(M, Cc))
        check(lib.mi_colsum_ordered(M, Cc, _p(x), ld_of(x), _p(out), _p(ws), ws.numel() * 4, _stream()), "mi_colsum_ordered")
        return
    if defer is not None and Cc % 4 == 0 and 4 <= Cc <= 1024 and _colsum_deferred(x, None, out, defer):
        return
    e0 = _probe_open()
    vec = Cc % 4 == 0 and 4 <= Cc <= 1024 and ld_of(x) % 4 == 0 and x.data_ptr() % 16 == 0 and x.dtype == torch.float32
    lib = load_library()
    if vec:       # float4 rows on a full grid, per-workgroup partial sums through the scratch buffer
        ws = _workspace(x.device, _cvt_colsum_ws(M, Cc))
        check(lib.mi_f32_to_bf16_colsum(M, Cc, _p(x), ld_of(x), None, 0, _p(out), _p(ws), ws.numel() * 4, _stream()), "mi_f32_to_bf16_colsum")
    else:
        check(lib.mi_colsum(M, Cc, _p(x), ld_of(x), _p(out), _stream()), "mi_colsum")
    if e0 is not None:
        _probe_close(e0, "cvt_colsum_kernel<false, true>" if vec else "colsum_kernel", 0.0, f"M{M} C{Cc}", M * Cc * _esz(x))


# --------------------------------------------------------------------------- norms
def _colsum_deferred(x, y16, out, defer):
    """partial rows of x's column sums (and the bf16 copy y16, if given) now, their sum into `out` with the queue's batched row sum;
    False: the tensor is too small for that (the caller takes the direct path)"""
    M, Cc = _rows(x), x.shape[-1]
    need = _cvt_colsum_ws(M, Cc)
    if M < 4096 or not need or x.dtype != torch.float32 or ld_of(x) % 4 or x.data_ptr() % 16:
        return False
    part = defer.rows_buffer(x.device, need // 4)
    rows = C.c_int(0)
    e0 = _probe_open()
    check(load_library().mi_f32_to_bf16_colsum_part(M, Cc, _p(x), ld_of(x), _p(y16), Cc, _p(part), need, C.byref(rows), _stream()),
          "mi_f32_to_bf16_colsum_part")
    if e0 is not None:
        _probe_close(e0, "cvt_colsum_kernel<true, true>" if y16 is not None else "cvt_colsum_kernel<false, true>", 0.0, f"M{M} C{Cc} (rows)",
                     M * Cc * (6.0 if y16 is not None else 4.0))
    assert rows.value > 0
    defer.push_rowsum(part, rows.value, Cc, Cc, out)
    return True


def to_bf16(x, colsum_out=None, defer=None):
    """bf16 copy (round-to-nearest-even) of an fp32 NHWC activation or channel slice: the MFMA operand of the next conv /
    weight gradient, rounded once for all of its consumers.  colsum_out (optional)[c] += sum over pixels of x[..., c] from the
    same pass (the bias gradient when x is a conv's output gradient); defer (a WgradQueue): the sums leave as partial rows and are
    added by the queue's batched row sum (no second pass per tensor)."""
    _need_gpu(x)
    N, H, W, Cc = x.shape
    y = new_act(N, H, W, Cc, x, torch.bfloat16)
    if colsum_out is not None and defer is not None and _colsum_deferred(x, y, colsum_out, defer):
        return y
    e0 = _probe_open()
    if colsum_out is not None:
        lib = load_library()
        ws = _workspace(x.device, _cvt_colsum_ws(N * H * W, Cc))
        check(lib.mi_f32_to_bf16_colsum(N * H * W, Cc, _p(x), ld_of(x), _p(y), Cc, _p(colsum_out), _p(ws), ws.numel() * 4, _stream()),
              "mi_f32_to_bf16_colsum")
    else:
        check(load_library().mi_f32_to_bf16(N * H * W, Cc, _p(x), ld_of(x), _p(y), Cc, _stream()), "mi_f32_to_bf16")
    if e0 is not None:
        _probe_close(e0, "cvt_colsum_kernel<true, true>" if colsum_out is not None else "f32_to_bf16_kernel", 0.0,
                     f"M{N * H * W} C{Cc}", N * H * W * Cc * 6.0)
    return y


def gn_mish_fwd(x, gamma, beta, *, groups=8, eps=1e-5, temb=None, residual=None, out_dtype=torch.float32, want16=False):
    """-> (y, stats), or (y, stats, y16) with want16: y16 = y rounded to bf16, written by the same pass."""
    _need_gpu(x)
    N, H, W, Cc = x.shape
    y = new_act(N, H, W, Cc, x, out_dtype)
    if want16:
        y16 = new_act(N, H, W, Cc, x, torch.bfloat16)
        stats = torch.empty((N, groups, 2), device=x.device, dtype=torch.float32)
        d = MiGnDesc(N=N, HW=H * W, C=Cc, G=groups, eps=eps, ldx=ld_of(x), ldy=ld_of(y), ldr=_ldn(residual))
        io = _b16(x) | (_b16(y) << 1)
        e0 = _probe_open()
        check(load_library().mi_gn_mish_fwd_dual(C.byref(d), _p(x), _p(gamma), _p(beta), _p(temb), ld_of(temb) if temb is not None else 0,
                                                 _p(residual), _p(y), _p(y16), Cc, _p(stats), io, _stream()), "mi_gn_mish_fwd_dual")
        if e0 is not None:
            _probe_close(e0, f"gn_mish_fwd_kernel<io{io}>", 0.0, f"N{N} HW{H * W} C{Cc} res{int(residual is not None)} +bf16 copy",
                         N * H * W * Cc * (_esz(x) + _esz(y) + _esz(residual) + 2))
        return y, stats, y16
    stats = torch.empty((N, groups, 2), device=x.device, dtype=torch.float32)
    d = MiGnDesc(N=N, HW=H * W, C=Cc, G=groups, eps=eps, ldx=ld_of(x), ldy=ld_of(y), ldr=_ldn(residual))
    io = _b16(x) | (_b16(y) << 1)
    ldt = ld_of(temb) if temb is not None else 0
    e0 = _probe_open()
    if io:
        check(load_library().mi_gn_mish_fwd_io(C.byref(d), _p(x), _p(gamma), _p(beta), _p(temb), ldt, _p(residual), _p(y),
                                               _p(stats), io, _stream()), "mi_gn_mish_fwd_io")
    else:
        check(load_library().mi_gn_mish_fwd(C.byref(d), _p(x), _p(gamma), _p(beta), _p(temb), ldt, _p(residual), _p(y),
                                            _p(stats), _stream()), "mi_gn_mish_fwd")
    if e0 is not None:
        _probe_close(e0, f"gn_mish_fwd_kernel<io{io}>", 0.0, f"N{N} HW{H * W} C{Cc} res{int(residual is not None)}",
                     N * H * W * Cc * (_esz(x) + _esz(y) + _esz(residual)))
    return y, stats


def gn_mish_bwd(x, stats, gamma, beta, dout, *, groups=8, eps=1e-5, dgamma=None, dbeta=None, dtemb=None, dbias=None,
                out_dtype=torch.float32):
    N, H, W, Cc = x.shape
    dx = new_act(N, H, W, Cc, x, out_dtype)
    d = MiGnDesc(N=N, HW=H * W, C=Cc, G=groups, eps=eps, ldx=ld_of(x), ldy=0, ldr=0)
    io = _b16(x) | (_b16(dx) << 1) | (_b16(dout) << 2)
    ldt = ld_of(dtemb) if dtemb is not None else 0
    e0 = _probe_open()
    if io:
        check(load_library().mi_gn_mish_bwd_io(C.byref(d), _p(x), _p(stats), _p(gamma), _p(beta), _p(dout), ld_of(dout),
                                               _p(dx), ld_of(dx), _p(dgamma), _p(dbeta), _p(dtemb), ldt, _p(dbias), io,
                                               _stream()), "mi_gn_mish_bwd_io")
    else:
        check(load_library().mi_gn_mish_bwd(C.byref(d), _p(x), _p(stats), _p(gamma), _p(beta), _p(dout), ld_of(dout),
                                            _p(dx), ld_of(dx), _p(dgamma), _p(dbeta), _p(dtemb), ldt, _p(dbias), _stream()),
              "mi_gn_mish_bwd")
    if e0 is not None:
        _probe_close(e0, f"gn_mish_bwd_kernel<io{io}>", 0.0, f"N{N} HW{H * W} C{Cc}", N * H * W * Cc * (_esz(x) + _esz(dout) + _esz(dx)))
    return dx


def chan_layernorm_fwd(x, g, b, eps=1e-5, out_dtype=torch.float32):
    _need_gpu(x)
    N, H, W, Cc = x.shape
    y = new_act(N, H, W, Cc, x, out_dtype)
    e0 = _probe_open()
    check(load_library().mi_chan_layernorm_fwd_io(N * H * W, Cc, _p(x), ld_of(x), _p(g), _p(b), eps, _p(y), ld_of(y), _b16(y),
                                                  _stream()), "mi_chan_layernorm_fwd")
    if e0 is not None:
        _probe_close(e0, f"chan_ln_fwd_kernel<io{_b16(y)}>", 0.0, f"M{N * H * W} C{Cc}", N * H * W * Cc * (_esz(x) + _esz(y)))
    return y


def ln_conv1x1_supported(N, H, W, K, Nc, ldx=None):
    """Does the LayerNorm + 1x1 conv kernel (mi_ln_conv1x1_pw) take the layer?"""
    return bool(_query("mi_ln_conv1x1_pw_supported", _conv_desc(N, H, W, K, Nc, 1, ldx=ldx)))


def ln_conv1x1(x, g, b, wq, *, Nc, eps=1e-5, bias=None, want_ln=False):
    """y = conv1x1(chan_layernorm(x)) as bf16 in ONE launch: PreNorm + to_qkv, reference src/models/ddpm.py:85-106,151.  x: the fp32
    residual stream [N, H, W, K], wq: the conv's slice of pack_weights_bf16's wfq.  Inference: the normalised tensor is never written;
    want_ln (training: to_qkv's weight gradient reads it): -> (y, ln), ln bf16, written by the same launch."""
    _need_gpu(x)
    assert x.dtype == torch.float32
    N, H, W, K = x.shape
    y = new_act(N, H, W, Nc, x, torch.bfloat16)
    ln = new_act(N, H, W, K, x, torch.bfloat16) if want_ln else None
    d = _conv_desc(N, H, W, K, Nc, 1, ldx=ld_of(x), ldy=ld_of(y))
    e0 = _probe_open()
    if want_ln:
        check(load_library().mi_ln_conv1x1_pw_dual(C.byref(d), _p(x), _p(g), _p(b), eps, _p(wq), _p(bias), _p(y), _p(ln), ld_of(ln), _stream()),
              "mi_ln_conv1x1_pw_dual")
    else:
        check(load_library().mi_ln_conv1x1_pw(C.byref(d), _p(x), _p(g), _p(b), eps, _p(wq), _p(bias), _p(y), _stream()), "mi_ln_conv1x1_pw")
    if e0 is not None:
        px, nch = (128 if (K == 128 and N * H * W // 128 >= 512) else 64), K // 128
        g2 = "true" if (px == 64 and N * H * W // 64 < 512) else "false"      # mi_ln_conv1x1_pw's pick, restated for the symbol name only
        _probe_close(e0, f"ln_conv1x1_pw_kernel<{px}, {nch}, {g2}>", 2.0 * N * H * W * Nc * K, f"N{N} {H}x{W} K{K}->{Nc} fp32 in + LayerNorm",
                     N * H * W * (K * 4 + Nc * 2 + (2 * K if want_ln else 0)) + K * Nc * 2)
    return (y, ln) if want_ln else y


def chan_layernorm_bwd(x, g, dy, dx, accumulate, dg, db, eps=1e-5, defer=None, dx_in=None):
    """defer (a WgradQueue): dg / db leave as one partial row per workgroup and are added by the queue's batched row sum -- the
    2 C atomics of every workgroup on the same addresses cost ~10 us per launch.
    dx_in (fp32, read only): dx = dx_in + gradient, out of place (mi_chan_layernorm_bwd_out; the bits of the accumulating in-place
    call) -- `accumulate` is then implied."""
    N, H, W, Cc = x.shape
    e0 = _probe_open()
    lib = load_library()
    if dx_in is not None:
        part = rows = None
        if defer is not None and dg is not None and db is not None:
            rows = lib.mi_chan_layernorm_bwd_part_rows(N * H * W, Cc)
            part = defer.rows_buffer(x.device, rows * 2 * Cc)
        check(lib.mi_chan_layernorm_bwd_out(N * H * W, Cc, _p(x), ld_of(x), _p(g), eps, _p(dy), ld_of(dy), _p(dx_in), ld_of(dx_in),
                                            _p(dx), ld_of(dx), None if part is not None else _p(dg), None if part is not None else _p(db),
                                            _p(part), _b16(dy), _stream()), "mi_chan_layernorm_bwd_out")
        if part is not None:
            defer.push_rowsum(part, rows, Cc, 2 * Cc, dg)
            defer.push_rowsum(part[Cc:], rows, Cc, 2 * Cc, db)
        accumulate = True
    elif defer is not None and dg is not None and db is not None:
        rows = lib.mi_chan_layernorm_bwd_part_rows(N * H * W, Cc)
        part = defer.rows_buffer(x.device, rows * 2 * Cc)
        check(lib.mi_chan_layernorm_bwd_part(N * H * W, Cc, _p(x), ld_of(x), _p(g), eps, _p(dy), ld_of(dy), _p(dx), ld_of(dx),
                                             int(accumulate), _p(part), _b16(dy), _stream()), "mi_chan_layernorm_bwd_part")
        defer.push_rowsum(part, rows, Cc, 2 * Cc, dg)
        defer.push_rowsum(part[Cc:], rows, Cc, 2 * Cc, db)
    else:
        check(lib.mi_chan_layernorm_bwd_io(N * H * W, Cc, _p(x), ld_of(x), _p(g), eps, _p(dy), ld_of(dy), _p(dx),
                                           ld_of(dx), int(accumulate), _p(dg), _p(db), _b16(dy), _stream()),
              "mi_chan_layernorm_bwd")
    if e0 is not None:
        _probe_close(e0, f"chan_ln_bwd_kernel<io{_b16(dy)}>", 0.0, f"M{N * H * W} C{Cc} acc{int(accumulate)}",
                     N * H * W * Cc * (_esz(x) + _esz(dy) + _esz(dx) * (2 if accumulate else 1)))


# --------------------------------------------------------------------------- nn.Linear of the time MLP (exact fp32)
def small_gemm(ta, tb, A, B, *, bias=None, out=None, accumulate=False, allow_split=False):
    """out[i][j] (+)= bias[j] + sum_k opA(i,k) opB(k,j) (mi_small_gemm); returns None when the shape is not supported.
    allow_split: long contractions may be split and combined with atomics (gradients; not bit-reproducible)."""
    _need_gpu(A)
    I = A.shape[1] if ta else A.shape[0]
    Kc = A.shape[0] if ta else A.shape[1]
    J = B.shape[0] if tb else B.shape[1]
    lib = load_library()
    if (A.dtype != torch.float32 or B.dtype != torch.float32 or A.stride(1) != 1 or B.stride(1) != 1 or
            (A.data_ptr() | B.data_ptr()) & 15 or not lib.mi_small_gemm_supported(int(ta), int(tb), I, J, Kc, A.stride(0), B.stride(0))):
        return None
    if out is None:
        assert not accumulate
        out = torch.empty((I, J), device=A.device, dtype=torch.float32)
    check(lib.mi_small_gemm(int(ta), int(tb), I, J, Kc, _p(A), A.stride(0), _p(B), B.stride(0), _p(bias), _p(out), out.stride(0),
                            int(accumulate), int(allow_split), _stream()), "mi_small_gemm")
    return out


# --------------------------------------------------------------------------- VQ-VAE codebook step (vqvae.py:24-43)
def vq_nearest(z_rows, codebook):
    """z_rows [M, D] (row stride % 4 == 0), codebook [K, D] -> (idx int32 [M], zq [M, D], sum ||z - zq||^2 as a 0-dim tensor)."""
    _need_gpu(z_rows)
    M, D = z_rows.shape
    Kc = codebook.shape[0]
    assert z_rows.stride(1) == 1 and codebook.is_contiguous() and codebook.shape[1] == D
    idx = torch.empty(M, device=z_rows.device, dtype=torch.int32)
    zq = torch.empty((M, D), device=z_rows.device, dtype=torch.float32)
    part = torch.empty(load_library().mi_vq_partials(M), device=z_rows.device, dtype=torch.float32)
    check(load_library().mi_vq_nearest_fwd(M, D, Kc, _p(z_rows), z_rows.stride(0), _p(codebook), _p(idx), _p(zq), D, _p(part), _stream()),
          "mi_vq_nearest_fwd")
    return idx, zq, part.sum()


def vq_backward(z_rows, codebook, idx, g_vq, g_commit, dz=None, accumulate=False, dcodebook=None, g_dev=None):
    """Adds the gradients of g_vq * vq_loss + g_commit * mean((z - sg(q))^2) into dz / dcodebook (either may be None);
    g_dev: optional 2-float device tensor multiplied into (g_vq, g_commit)."""
    M, D = z_rows.shape
    check(load_library().mi_vq_bwd(M, D, codebook.shape[0], _p(z_rows), z_rows.stride(0), _p(codebook), _p(idx), float(g_vq), float(g_commit),
                                   _p(g_dev), _p(dz), dz.stride(0) if dz is not None else 0, int(accumulate), _p(dcodebook), _stream()), "mi_vq_bwd")


def vq_scatter_rows(src_rows, idx, table):
    """table[idx[m]] += src_rows[m]."""
    M, D = src_rows.shape
    check(load_library().mi_vq_scatter_rows(M, D, table.shape[0], _p(src_rows), src_rows.stride(0), _p(idx), _p(table), _stream()),
          "mi_vq_scatter_rows")


# --------------------------------------------------------------------------- attention
def linattn_fwd(qkv, heads=4):
    _need_gpu(qkv)
    N, H, W, C3 = qkv.shape
    assert C3 == 3 * heads * 32 and qkv.is_contiguous()
    out = new_act(N, H, W, heads * 32, qkv, qkv.dtype)        # bf16 qkv -> bf16 output (attention-internal storage)
    ctx = torch.empty((N, heads, 32, 32), device=qkv.device, dtype=torch.float32)
    kstat = torch.empty((N, heads, 32, 2), device=qkv.device, dtype=torch.float32)
    e0 = _probe_open()
    lib = load_library()
    need = _linattn_ws(N, H * W, heads)                      # > 0: the pixel axis is cut into slices (several workgroups per image)
    ws = _workspace(qkv.device, need) if need else None
    check(lib.mi_linattn_fwd_ws(N, H * W, heads, _p(qkv), _p(out), _p(ctx), _p(kstat), _b16(qkv), _p(ws), ws.numel() * 4 if need else 0,
                                _stream()), "mi_linattn_fwd")
    if e0 is not None:
        _probe_close(e0, f"linattn_fwd_kernel<io{_b16(qkv)}>", 4.0 * N * heads * 32 * 32 * H * W, f"N{N} n{H * W}",
                     N * H * W * heads * 32 * 4 * _esz(qkv))
    return out, ctx, kstat


def linattn_to_out_folded(qkv, w_out16, Cc, bias, residual, heads=4, want16=False):
    """Inference: LinearAttention + its to_out conv + the Residual add (reference ddpm.py:146-165, Residual) as TWO launches that never form the
    attention output: (1) mi_linattn_fold_fwd -- softmax statistics and context per (sample, head) as in linattn_fwd, then the per-sample
    effective weights W_eff[b] = W_out blockdiag(ctx_h^T) in fragment order; (2) mi_conv1x1_pw_batched -- y = W_eff[b] q + bias + residual,
    q read straight out of qkv.  qkv bf16 [N, H, W, 3 * heads * 32], w_out16: to_out's bf16 weight rows [C][heads * 32] (pack_weights_bf16's wf slice).
    -> y fp32 (want16: (y, its bf16 copy)); None when the shape is not taken."""
    _need_gpu(qkv)
    N, H, W, C3 = qkv.shape
    hid = heads * 32
    if (qkv.dtype != torch.bfloat16 or C3 != 3 * hid or not qkv.is_contiguous() or hid % 128 or Cc % 64 or (H * W) % 64 or (N * H * W) % 128
            or _linattn_ws(N, H * W, heads)):
        return None
    lib = load_library()
    weff = torch.empty((N, Cc * hid), device=qkv.device, dtype=torch.bfloat16)
    e0 = _probe_open()
    check(lib.mi_linattn_fold_fwd(N, H * W, heads, _p(qkv), _p(w_out16), Cc, _p(weff), _stream()), "mi_linattn_fold_fwd")
    if e0 is not None:
        _probe_close(e0, "linattn_fwd_kernel<io1, fold>", 2.0 * N * heads * 32 * 32 * (H * W + Cc), f"N{N} n{H * W} C{Cc}",
                     N * H * W * 2 * hid * 2 + N * Cc * hid * 2)
    y = new_act(N, H, W, Cc, qkv, torch.float32)
    y16 = new_act(N, H, W, Cc, qkv, torch.bfloat16) if want16 else None
    d = _conv_desc(N, H, W, hid, Cc, 1, ldx=C3, ldy=ld_of(y), ldr=_ldn(residual))
    e0 = _probe_open()
    check(lib.mi_conv1x1_pw_batched(C.byref(d), _p(qkv), _p(weff), Cc * hid, _p(bias), _p(residual), _p(y), 0, _p(y16),
                                    ld_of(y16) if y16 is not None else 0, _stream()), "mi_conv1x1_pw_batched")
    if e0 is not None:
        px = 64 if ((N * H * W // 128) * ((Cc + 127) // 128) < 256 or (H * W) % 128) else 128
        _probe_close(e0, f"conv1x1_pw_kernel<false, {'true' if want16 else 'false'}, {px}>", 2.0 * N * H * W * Cc * hid,
                     f"N{N} {H}x{W} K{hid}->{Cc} per-sample weights", N * H * W * (hid * 2 + Cc * (4 + _esz(residual) + (2 if want16 else 0))) + N * Cc * hid * 2)
    return (y, y16) if want16 else y


def linattn_bwd(qkv, ctx, kstat, dout, heads=4):
    N, H, W, C3 = qkv.shape
    assert dout.is_contiguous() and dout.dtype == qkv.dtype
    dqkv = torch.empty_like(qkv)
    e0 = _probe_open()
    lib = load_library()
    need = _linattn_ws(N, H * W, heads)
    ws = _workspace(qkv.device, need) if need else None
    check(lib.mi_linattn_bwd_ws(N, H * W, heads, _p(qkv), _p(ctx), _p(kstat), _p(dout), _p(dqkv), _b16(qkv), _p(ws),
                                ws.numel() * 4 if need else 0, _stream()), "mi_linattn_bwd")
    if e0 is not None:
        _probe_close(e0, f"linattn_bwd_kernel<io{_b16(qkv)}>", 12.0 * N * heads * 32 * 32 * H * W, f"N{N} n{H * W}",
                     N * H * W * heads * 32 * 7 * _esz(qkv))
    return dqkv


# --------------------------------------------------------------------------- element-wise
def time_embed(t, dim):
    if not t.is_cuda:
        raise RuntimeError("time_embed needs a GPU tensor")
    t = t.to(torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), device=t.device, dtype=torch.float32)
    check(load_library().mi_time_embed(t.shape[0], dim, _p(t), _p(out), _stream()), "mi_time_embed")
    return out


def mish_fwd(x):
    _need_gpu(x)
    y = torch.empty_like(x)
    check(load_library().mi_mish_fwd(x.numel(), _p(x), _p(y), _stream()), "mi_mish_fwd")
    return y


def mish_bwd(x, dy):
    dx = torch.empty_like(x)
    check(load_library().mi_mish_bwd(x.numel(), _p(x), _p(dy), _p(dx), _stream()), "mi_mish_bwd")
    return dx


def relu_fwd(x, inplace=False):
    """max(x, 0) on a dense tensor (any shape); inplace mirrors nn.ReLU(True)."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == torch.float32
    y = x if inplace else torch.empty_like(x)
    check(load_library().mi_relu_fwd(x.numel(), _p(x), _p(y), _stream()), "mi_relu_fwd")
    return y


def relu_bwd(y, dy, out=None, accumulate=False):
    """dx (+)= dy where the ReLU OUTPUT y is positive; out=None allocates, out=dy works in place."""
    assert y.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(dy) if out is None else out
    check(load_library().mi_relu_bwd(y.numel(), _p(y), _p(dy), _p(dx), int(accumulate), _stream()), "mi_relu_bwd")
    return dx


# --------------------------------------------------------------------------- VAE operators (vae_ops.hip)
_BN_WS = {}


def _bn_ws(device, C):
    ws = _BN_WS.get(device)
    if ws is None or ws.numel() < 2 * C:
        ws = torch.zeros(max(2 * C, 4096), device=device, dtype=torch.float64)     # kept zero by the kernels
        _BN_WS[device] = ws
    return ws


def batchnorm_fwd(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True):
    """nn.BatchNorm2d on a dense NHWC tensor -> (y, mean[C], rstd[C]); updates the running statistics in training mode."""
    _need_gpu(x); _dense(x)
    Cc = x.shape[-1]
    M = x.numel() // Cc
    y = torch.empty_like(x)
    mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
    rstd = torch.empty(Cc, device=x.device, dtype=torch.float32)
    check(load_library().mi_batchnorm_fwd(M, Cc, _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), _p(running_mean), _p(running_var),
                                          momentum, eps, int(training), _p(_bn_ws(x.device, Cc)), _stream()), "mi_batchnorm_fwd")
    return y, mean, rstd


def batchnorm_bwd(x, mean, rstd, gamma, dy, dgamma=None, dbeta=None, out=None):
    _dense(x, dy, out)
    Cc = x.shape[-1]
    M = x.numel() // Cc
    dx = torch.empty_like(x) if out is None else out
    check(load_library().mi_batchnorm_bwd(M, Cc, _p(x), _p(mean), _p(rstd), _p(gamma), _p(dy), _p(dx), _p(dgamma), _p(dbeta),
                                          _p(_bn_ws(x.device, Cc)), _stream()), "mi_batchnorm_bwd")
    return dx


def vae_latent_fwd(h, eps):
    """h [N, 2L] = [mu | log_sigma], eps [N, L] -> (z [N, L], kld scalar)."""
    _need_gpu(h)
    N, L2 = h.shape
    L = L2 // 2
    z = torch.empty((N, L), device=h.device, dtype=torch.float32)
    kld = torch.zeros((), device=h.device, dtype=torch.float32)
    eps = eps.float().contiguous()
    check(load_library().mi_vae_latent_fwd(N, L, _p(h), h.stride(0), _p(eps), _p(z), _p(kld), _stream()), "mi_vae_latent_fwd")
    return z, kld


def vae_latent_bwd(h, eps, dz, g_kld, g_dev=None):
    N, L2 = h.shape
    dh = torch.empty((N, L2), device=h.device, dtype=torch.float32)
    check(load_library().mi_vae_latent_bwd(N, L2 // 2, _p(h), h.stride(0), _p(eps.float().contiguous()), _p(dz.contiguous()), float(g_kld), _p(g_dev),
                                           _p(dh), L2, _stream()), "mi_vae_latent_bwd")
    return dh


# --------------------------------------------------------------------------- cVAE operators (cvae_ops.hip)
def _labels_i64(labels, like):
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int64 and labels.device == like.device):
        raise RuntimeError("labels: an int64 tensor on the images' HIP device is expected")
    return labels.contiguous()


def cvae_pack_input(x, labels, ncls):
    """NCHW images + int64 labels [N] -> the encoder's NHWC input [N, H, W, C + ncls] = [image | one-hot label planes], a view of a
    buffer whose pixel pitch ceil4(C + ncls) is zero in its padding lanes (one launch: no one-hot tensor, no cat)."""
    _need_gpu(x)
    B, Cc, H, W = x.shape
    labels = _labels_i64(labels, x)
    assert labels.shape == (B,)
    ld = (Cc + ncls + 3) // 4 * 4
    x = x.contiguous()
    y = torch.empty((B, H, W, ld), device=x.device, dtype=torch.float32)
    check(load_library().mi_cvae_pack_input(B, Cc, H * W, ncls, _p(x), _p(labels), _p(y), ld, _stream()), "mi_cvae_pack_input")
    return y[..., :Cc + ncls]


def cvae_latent_fwd(h, eps, labels, E):
    """h [N, 2L] = [mu | log_sigma], eps [N, L], E [ncls, L] -> (zc [N, 2L] = [mu + exp(log_sigma) eps | E[labels]], kld scalar).
    h None: eps holds z and the call only concatenates -> (zc, None)."""
    _need_gpu(eps)
    N, L = eps.shape
    labels = _labels_i64(labels, eps)
    assert labels.shape == (N,) and E.shape[1] == L and E.is_contiguous() and (h is None or h.shape == (N, 2 * L))
    eps = eps.float().contiguous()
    zc = torch.empty((N, 2 * L), device=eps.device, dtype=torch.float32)
    kld = torch.empty((), device=eps.device, dtype=torch.float32) if h is not None else None
    check(load_library().mi_cvae_latent_fwd(N, L, E.shape[0], _p(h), h.stride(0) if h is not None else 0, _p(eps), _p(labels), _p(E),
                                            _p(zc), _p(kld), _stream()), "mi_cvae_latent_fwd")
    return zc, kld


def cvae_latent_bwd(h, eps, labels, dzc, g_kld, dE, g_dev=None):
    """dh [N, 2L] from dzc [N, 2L] (its first half is dL/dz); dE [ncls, L] += the label-segmented sum of dzc's second half."""
    N, L2 = h.shape
    L = L2 // 2
    labels = _labels_i64(labels, h)
    assert dzc.shape == (N, L2) and dzc.stride(1) == 1 and dE.shape[1] == L and dE.is_contiguous()
    dh = torch.empty((N, L2), device=h.device, dtype=torch.float32)
    check(load_library().mi_cvae_latent_bwd(N, L, dE.shape[0], _p(h), h.stride(0), _p(eps.float().contiguous()), _p(labels), _p(dzc),
                                            dzc.stride(0), float(g_kld), _p(g_dev), _p(dh), _p(dE), _stream()), "mi_cvae_latent_bwd")
    return dh


# --------------------------------------------------------------------------- latent discriminator (latent_disc.hip)
LATENT_DISC_H = 256


def latent_disc_supported(N, L, H=LATENT_DISC_H) -> bool:
    return load_library().mi_latent_disc_supported(int(N), int(L), int(H)) == 1


def _ld_ptrs(ts):
    assert len(ts) == 10
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("latent discriminator: parameters / gradients are dense float32 tensors on the HIP device")
    return (C.c_void_p * 10)(*[t.data_ptr() for t in ts])


def _ld_source(z, h, eps, perm):
    """-> (N, L, the eight source arguments of the C ABI, tensors to keep alive)."""
    if z is not None:
        if h is not None or eps is not None or perm is not None:
            raise RuntimeError("latent discriminator input: either z, or h + eps (+ perm)")
        _need_gpu(z)
        if z.dim() != 2 or z.stride(1) != 1 or z.dtype != torch.float32:
            raise RuntimeError("z: float32 rows with unit column stride")
        N, L = z.shape
        return N, L, (_p(z), z.stride(0), _p(None), 0, _p(None), _p(None)), (z,)
    if h is None or eps is None:
        raise RuntimeError("latent discriminator input: either z, or h + eps (+ perm)")
    _need_gpu(h)
    _need_gpu(eps)
    N, L = eps.shape
    if h.dim() != 2 or h.shape[0] != N or h.shape[1] < 2 * L or h.stride(1) != 1 or h.dtype != torch.float32 or eps.dtype != torch.float32:
        raise RuntimeError("h: float32 rows [mu | log_sigma] of at least 2 L columns, one per row of eps")
    eps = eps.contiguous()
    if perm is not None:
        if not (torch.is_tensor(perm) and perm.is_cuda and perm.dtype == torch.int64 and perm.device == h.device and perm.shape == (L, N)):
            raise RuntimeError("perm: an int64 tensor [L, N] on the latents' HIP device is expected")
        perm = perm.contiguous()
    return N, L, (_p(None), 0, _p(h), h.stride(0), _p(eps), _p(perm)), (h, eps, perm)


def latent_disc_fwd(params, target, z=None, h=None, eps=None, perm=None, training=True, running_mean=None, running_var=None,
                    num_batches_tracked=None, momentum=0.1):
    """MLPEncoder(L, [256, 256], 1) + least-squares loss in two launches.  params: the ten tensors in the C ABI's order (weights
    input-major).  Input: z [N, L] rows | h [N, >= 2L] + eps [N, L] (x = mu + exp(log_sigma) eps) | those + perm int64 [L, N]
    (x[n, j] = z[perm[j, n], j]).  Returns a record: logit [N], loss, mean_logit and mean_sq_logit (device scalars; the last is the loss against target 0) and what `latent_disc_bwd` needs."""
    N, L, src, keep = _ld_source(z, h, eps, perm)
    lib = load_library()
    if lib.mi_latent_disc_supported(N, L, LATENT_DISC_H) != 1:
        check(-1, "mi_latent_disc_supported")
    dev = keep[0].device
    tape = torch.empty(lib.mi_latent_disc_tape_floats(N), device=dev, dtype=torch.float32)
    out3 = torch.empty(3, device=dev, dtype=torch.float32)
    if not training and (running_mean is None or running_var is None):
        raise RuntimeError("evaluation mode needs the running statistics")
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise RuntimeError("num_batches_tracked: int64")
    check(lib.mi_latent_disc_fwd(N, L, LATENT_DISC_H, *src, _ld_ptrs(params), int(bool(training)), float(target), float(momentum),
                                 _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(tape), _p(out3), _stream()),
          "mi_latent_disc_fwd")
    return {"N": N, "L": L, "src": src, "keep": keep, "training": bool(training), "tape": tape, "out3": out3, "logit": tape[tape.numel() - N:],
            "loss": out3[0], "mean_logit": out3[1], "mean_sq_logit": out3[2]}


def latent_disc_bwd(params, rec, target, grads=None, param_scale=1.0, accumulate_params=False, dz=None, dz_scale=1.0, accumulate_dz=False):
    """Backward of mean((logit - target)^2) from a forward record (3 launches, 2 without parameter gradients).
    grads: ten tensors like params, g = (accumulate_params ? g : 0) + param_scale * gradient;  dz: [N, L] rows with unit column
    stride, dz = (accumulate_dz ? dz : 0) + dz_scale * d loss / d x.  Returns dz."""
    N, L = rec["N"], rec["L"]
    lib = load_library()
    if grads is None and dz is None:
        raise RuntimeError("latent_disc_bwd: neither parameter gradients nor an input gradient asked for")
    lddz = 0
    if dz is not None:
        _need_gpu(dz)
        if dz.shape != (N, L) or dz.stride(1) != 1 or dz.dtype != torch.float32:
            raise RuntimeError("dz: float32 [N, L] rows with unit column stride")
        lddz = dz.stride(0)
    ws = torch.empty(lib.mi_latent_disc_workspace_floats(N), device=rec["tape"].device, dtype=torch.float32)
    check(lib.mi_latent_disc_bwd(N, L, LATENT_DISC_H, *rec["src"], _ld_ptrs(params), int(rec["training"]), float(target), _p(rec["tape"]),
                                 _p(ws), _ld_ptrs(grads) if grads is not None else None, float(param_scale), int(bool(accumulate_params)),
                                 _p(dz), lddz, float(dz_scale), int(bool(accumulate_dz)), _stream()), "mi_latent_disc_bwd")
    return dz


# --------------------------------------------------------------------------- row-local latent discriminator (latent_disc_ln.hip)
LATENT_DISC_LN_LOSSES = {"vanilla": 0, "lsgan": 1}


def latent_disc_ln_supported(N0, N1, L, H=LATENT_DISC_H) -> bool:
    return load_library().mi_latent_disc_ln_supported(int(N0), int(N1), int(L), int(H)) == 1


def _ldl_rows(x, what):
    _need_gpu(x)
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 rows [N, L] with unit column stride")
    return x


def latent_disc_ln_fwd(params, x0, target0, x1=None, target1=0.0, loss_mode="vanilla"):
    """MLPEncoder(L, [256, 256], 1, norm_type="layer") + the adversarial loss in two launches.  params: the ten tensors in the C ABI's
    order (weights input-major).  x0 [N0, L] against target0 and (optionally) x1 [N1, L] against target1 go through as ONE pass of
    N0 + N1 rows; both may be pitched views.  Returns a record: logit [N0 + N1], loss0, loss1, mean_logit0, mean_logit1, d_loss =
    0.5 (loss0 + loss1) (device scalars) and what `latent_disc_ln_bwd` needs."""
    x0 = _ldl_rows(x0, "x0")
    N0, L = x0.shape
    N1 = 0
    if x1 is not None:
        x1 = _ldl_rows(x1, "x1")
        if x1.shape[1] != L or x1.device != x0.device:
            raise RuntimeError("x1: rows of the same width and on the same device as x0")
        N1 = x1.shape[0]
        if N1 == 0:
            x1 = None
    mode = LATENT_DISC_LN_LOSSES.get(loss_mode)
    if mode is None:
        raise RuntimeError(f"loss_mode={loss_mode!r}: 'vanilla' or 'lsgan'")
    lib = load_library()
    if lib.mi_latent_disc_ln_supported(N0, N1, L, LATENT_DISC_H) != 1:
        check(-1, "mi_latent_disc_ln_supported")
    N = N0 + N1
    tape = torch.empty(lib.mi_latent_disc_ln_tape_floats(N), device=x0.device, dtype=torch.float32)
    out5 = torch.empty(5, device=x0.device, dtype=torch.float32)
    src = (N0, N1, L, LATENT_DISC_H, _p(x0), x0.stride(0) if N0 > 1 else max(L, x0.stride(0)), _p(x1),
           0 if x1 is None else (x1.stride(0) if N1 > 1 else max(L, x1.stride(0))))
    check(lib.mi_latent_disc_ln_fwd(*src, _ld_ptrs(params), mode, float(target0), float(target1), _p(tape), _p(out5), _stream()),
          "mi_latent_disc_ln_fwd")
    return {"N0": N0, "N1": N1, "L": L, "src": src, "keep": (x0, x1), "mode": mode, "tape": tape, "out5": out5,
            "logit": tape[3 * N * LATENT_DISC_H + 2 * N:3 * N * LATENT_DISC_H + 3 * N], "loss0": out5[0], "loss1": out5[1],
            "mean_logit0": out5[2], "mean_logit1": out5[3], "d_loss": out5[4]}


def latent_disc_ln_bwd(params, rec, target0, target1=0.0, c0=1.0, c1=0.0, grads=None, param_scale=1.0, accumulate_params=False, dx0=None,
                       dx_scale=1.0, accumulate_dx=False):
    """Backward of c0 loss0 + c1 loss1 against (target0, target1) from a forward record: 2 launches, 1 without parameter gradients.
    grads: ten tensors like params, g = (accumulate_params ? g : 0) + param_scale * gradient;  dx0: [N0, L] rows with unit column
    stride (the first segment's input gradient), dx0 = (accumulate_dx ? dx0 : 0) + dx_scale * gradient.  Returns dx0."""
    N0, N1, L = rec["N0"], rec["N1"], rec["L"]
    lib = load_library()
    if grads is None and dx0 is None:
        raise RuntimeError("latent_disc_ln_bwd: neither parameter gradients nor an input gradient asked for")
    lddx = 0
    if dx0 is not None:
        _need_gpu(dx0)
        if dx0.shape != (N0, L) or dx0.stride(1) != 1 or dx0.dtype != torch.float32:
            raise RuntimeError("dx0: float32 [N0, L] rows with unit column stride")
        lddx = dx0.stride(0) if N0 > 1 else max(L, dx0.stride(0))
    ws = None
    if grads is not None:
        ws = torch.empty(lib.mi_latent_disc_ln_workspace_floats(N0 + N1), device=rec["tape"].device, dtype=torch.float32)
    check(lib.mi_latent_disc_ln_bwd(*rec["src"], _ld_ptrs(params), rec["mode"], float(target0), float(target1), float(c0), float(c1),
                                    _p(rec["tape"]), _p(ws), _ld_ptrs(grads) if grads is not None else None, float(param_scale),
                                    int(bool(accumulate_params)), _p(dx0), lddx, float(dx_scale), int(bool(accumulate_dx)), _stream()),
          "mi_latent_disc_ln_bwd")
    return dx0


# --------------------------------------------------------------------------- BiGAN's pair head (pair_disc.hip)
PAIR_DISC_H = 128


def pair_disc_supported(N, L, H=PAIR_DISC_H, training=True) -> bool:
    """N: rows per segment.  Training mode needs two (BatchNorm1d), evaluation mode one."""
    return load_library().mi_pair_disc_supported(int(N), int(L), int(H), int(bool(training))) == 1


def _pd_ptrs(ts, aligned):
    if len(ts) != 16:
        raise RuntimeError("pair head: sixteen parameter / gradient tensors (dis_z's ten, dis_pair's six)")
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("pair head: parameters / gradients are dense float32 tensors on the HIP device")
        if aligned and t.data_ptr() % 16:
            raise RuntimeError("pair head: parameter tensors are 16-byte aligned")
    return (C.c_void_p * 16)(*[t.data_ptr() for t in ts])


def _pd_rows(x, rows, cols, what):
    _need_gpu(x)
    if x.dim() != 2 or x.shape != (rows, cols) or x.stride(1) != 1 or x.dtype != torch.float32 or (rows > 1 and x.stride(0) < cols):
        raise RuntimeError(f"{what}: float32 rows [{rows}, {cols}] with unit column stride and a pitch of at least {cols}")
    return x.stride(0) if rows > 1 else max(cols, x.stride(0))


def pair_disc_fwd(params, e, z, xf, loss_mode="vanilla", training=True, running_mean=None, running_var=None, num_batches_tracked=None,
                  momentum=0.1):
    """BiGAN's discriminator behind dis_x, on 2 N rows as two segments, and both adversarial losses, in three launches.  params: the
    sixteen tensors in the C ABI's order (weights input-major).  e [N, L]: segment 0's code rows (the encoder's output), z [N, L]:
    segment 1's, xf [2N, H]: dis_x's output rows; all may be pitched views, read in place.  Training mode: BatchNorm1d statistics per
    segment, the running statistics updated twice (segment 0 first), the counter += 2.  Returns a record: logit, dlogit_g, dlogit_d
    [2N]; g_loss, d_loss, mean_real, mean_fake, d_loss_real, d_loss_fake (device scalars); and what `pair_disc_bwd` needs."""
    _need_gpu(e)
    if e.dim() != 2 or z.dim() != 2 or xf.dim() != 2:
        raise RuntimeError("pair head: e [N, L], z [N, L] and xf [2N, H] are matrices")
    N, L = e.shape
    lde, ldz, ldf = _pd_rows(e, N, L, "e"), _pd_rows(z, N, L, "z"), _pd_rows(xf, 2 * N, PAIR_DISC_H, "xf")
    if z.device != e.device or xf.device != e.device:
        raise RuntimeError("pair head: e, z and xf live on one device")
    mode = ADV_LOSSES.get(loss_mode)
    if mode is None:
        raise NotImplementedError(f"loss_mode={loss_mode!r}: 'vanilla', 'lsgan' or 'hinge'")
    lib = load_library()
    if lib.mi_pair_disc_supported(N, L, PAIR_DISC_H, int(bool(training))) != 1:
        check(-1, "mi_pair_disc_supported")
    if not training and (running_mean is None or running_var is None):
        raise RuntimeError("evaluation mode needs the running statistics")
    for b in (running_mean, running_var):
        if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.shape == (PAIR_DISC_H,) and b.is_contiguous()):
            raise RuntimeError("running statistics: dense float32 [H] on the HIP device")
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise RuntimeError("num_batches_tracked: int64")
    dev = e.device
    tape = torch.empty(lib.mi_pair_disc_tape_floats(N, PAIR_DISC_H), device=dev, dtype=torch.float32)
    ws = torch.empty(lib.mi_pair_disc_workspace_floats(N, PAIR_DISC_H), device=dev, dtype=torch.float32)
    out = torch.empty((3, 2 * N), device=dev, dtype=torch.float32)
    out6 = torch.empty(6, device=dev, dtype=torch.float32)
    src = (N, L, PAIR_DISC_H, _p(e), lde, _p(z), ldz, _p(xf), ldf)
    check(lib.mi_pair_disc_fwd(*src, _pd_ptrs(params, True), int(bool(training)), mode, float(momentum), _p(running_mean), _p(running_var),
                               _p(num_batches_tracked), _p(tape), _p(ws), _p(out[0]), _p(out[1]), _p(out[2]), _p(out6), _stream()),
          "mi_pair_disc_fwd")
    _count_launches(2)
    return {"N": N, "L": L, "src": src, "keep": (e, z, xf), "training": bool(training), "mode": mode, "tape": tape, "out6": out6,
            "logit": out[0], "dlogit_g": out[1], "dlogit_d": out[2], "g_loss": out6[0], "d_loss": out6[1], "mean_real": out6[2],
            "mean_fake": out6[3], "d_loss_real": out6[4], "d_loss_fake": out6[5]}


def pair_disc_bwd(params, rec, dxf=None, de=None, in_scale=1.0, accumulate_in=False, grads=None, dxf_d=None, param_scale=1.0,
                  accumulate_params=False):
    """Backward from a `pair_disc_fwd` record.  Input gradients (from dlogit_g; dxf given): dxf [2N, H] rows (a pitched view will do)
    and de [N, L] (optional, segment 0's code gradient) = (accumulate_in ? old : 0) + in_scale * gradient -- 2 launches, 1 without de.
    Parameter gradients (from dlogit_d; grads given): sixteen tensors like params, g = (accumulate_params ? g : 0) + param_scale *
    gradient, and dxf_d [2N, H] dense (optional) = d d_loss / d xf -- 3 launches.  Both in one call: 3 launches, the same bits."""
    N, L = rec["N"], rec["L"]
    lib = load_library()
    if dxf is None and grads is None:
        raise RuntimeError("pair_disc_bwd: neither input gradients (dxf) nor parameter gradients (grads) asked for")
    if de is not None and dxf is None:
        raise RuntimeError("pair_disc_bwd: de comes with dxf")
    lddxf = ldde = 0
    if dxf is not None:
        lddxf = _pd_rows(dxf, 2 * N, PAIR_DISC_H, "dxf")
    if de is not None:
        ldde = _pd_rows(de, N, L, "de")
    if dxf_d is not None:
        _need_gpu(dxf_d)
        if grads is None or dxf_d.shape != (2 * N, PAIR_DISC_H) or dxf_d.dtype != torch.float32 or not dxf_d.is_contiguous():
            raise RuntimeError("dxf_d: dense float32 [2N, H], together with grads")
    ws = torch.empty(lib.mi_pair_disc_workspace_floats(N, PAIR_DISC_H), device=rec["tape"].device, dtype=torch.float32)
    check(lib.mi_pair_disc_bwd(*rec["src"], _pd_ptrs(params, True), int(rec["training"]), _p(rec["tape"]), _p(ws), _p(rec["dlogit_g"]),
                               _p(rec["dlogit_d"]), _p(dxf), lddxf, _p(de), ldde, float(in_scale), int(bool(accumulate_in)),
                               _pd_ptrs(grads, False) if grads is not None else None, _p(dxf_d), float(param_scale),
                               int(bool(accumulate_params)), _stream()), "mi_pair_disc_bwd")
    _count_launches((2 if grads is not None else (1 if de is not None else 0)))
    return dxf, de


# --------------------------------------------------------------------------- plain GAN operators (bn_seg.hip)
BN_SEG_ACTS = {None: 0, "none": 0, "relu": 1, "leaky_relu": 2}
ADV_LOSSES = {"vanilla": 0, "lsgan": 1, "hinge": 2}
_BN_SEG_WS = {}


def _bn_seg_ws(device, S, M, Cc):
    """The partial-sums workspace: any content will do (every slot a call reads, it wrote), so one buffer per device is reused."""
    need = load_library().mi_bn_seg_workspace(S, M, Cc)
    if need == 0:
        raise RuntimeError(f"bn_seg: S={S}, M={M}, C={Cc} is not covered (C % 4 == 0, C/4 a power of two <= 256)")
    ws = _BN_SEG_WS.get(device)
    if ws is None or ws.numel() * 8 < need:
        ws = torch.empty(max(need // 8, 1 << 16), device=device, dtype=torch.float64)
        _BN_SEG_WS[device] = ws
    return ws


def _bn_seg_shape(x, segments):
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    S = int(segments)
    if S < 1 or rows % S != 0 or x.shape[0] % S != 0:
        raise RuntimeError(f"segments={segments}: the {x.shape[0]} samples do not split into that many equal segments")
    return S, rows // S, Cc


def bn_seg_fwd(x, gamma, beta, segments=1, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True, act=None, slope=0.2):
    """nn.BatchNorm2d + activation on a dense NHWC tensor whose leading dimension holds `segments` equal batches, each with its own
    batch statistics and its own running-statistics update (segment 0 first) -> (y, mean[S, C], rstd[S, C]).  Two launches; one in
    evaluation mode, where every segment uses the running statistics.  act: None, "relu" or "leaky_relu" (slope)."""
    _need_gpu(x); _dense(x)
    S, M, Cc = _bn_seg_shape(x, segments)
    y = torch.empty_like(x)
    mean = torch.empty((S, Cc), device=x.device, dtype=torch.float32)
    rstd = torch.empty((S, Cc), device=x.device, dtype=torch.float32)
    ws = _bn_seg_ws(x.device, S, M, Cc) if training else None
    check(load_library().mi_bn_seg_fwd(S, M, Cc, _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), _p(running_mean), _p(running_var),
                                       momentum, eps, int(bool(training)), BN_SEG_ACTS[act], slope, _p(ws), _stream()), "mi_bn_seg_fwd")
    return y, mean, rstd


def bn_seg_bwd(x, mean, rstd, gamma, y, dy, act=None, slope=0.2, dgamma=None, dbeta=None, accumulate=False, out=None):
    """Backward of `bn_seg_fwd` in training mode from its input x, its saved statistics and its activated output y; the segment count
    is mean's leading dimension.  dx (out=dy works in place); dgamma / dbeta (optional) are stored, or added to with accumulate."""
    _need_gpu(x); _dense(x, y, dy, out)
    S, M, Cc = _bn_seg_shape(x, mean.shape[0])
    dx = torch.empty_like(x) if out is None else out
    check(load_library().mi_bn_seg_bwd(S, M, Cc, _p(x), _p(mean), _p(rstd), _p(gamma), _p(y), _p(dy), _p(dx), _p(dgamma), _p(dbeta),
                                       int(bool(accumulate)), BN_SEG_ACTS[act], slope, _p(_bn_seg_ws(x.device, S, M, Cc)), _stream()),
          "mi_bn_seg_bwd")
    return dx


def adv_loss(logit, targets, loss_mode="vanilla", scale=1.0, want_grad=True, dlogit_out=None):
    """The reference's adversarial_loss (src/utils/losses.py:4-24) per segment of the logits: targets = one bool per segment (True:
    "real").  logit: [N] or a discriminator's NHWC output [N, 1, 1, 1] (a view of a padded buffer: its pitch goes to the kernel).
    Returns (loss[S], mean_logit[S], dlogit) with dlogit = scale * d loss_s / d logit, shaped like logit -- for an NHWC logit a view
    of a zero-padded [N, 1, 1, 4] buffer, what the convolutions' backward reads -- or None.  "hinge" is the reference's formula:
    max(1 - x, 1) for real targets.  dlogit_out: N rows of a zero-padded [.., 1, 1, 4] buffer the caller holds, written instead of a new
    one (the VAE-GAN fills some segments of a longer gradient and leaves the others zero)."""
    _need_gpu(logit)
    mode = ADV_LOSSES.get(loss_mode)
    if mode is None:
        raise NotImplementedError(f"loss_mode={loss_mode!r}: 'vanilla', 'lsgan' or 'hinge'")
    return _adv_loss(logit, targets, mode, scale, want_grad, dlogit_out)


_WASSERSTEIN = 3        # mi_adv_loss' mode 3; not a `loss_mode` of the GAN, so not in ADV_LOSSES


def critic_loss(logit, targets, scale=1.0, want_grad=True):
    """The WGAN critic's loss per segment of the logits, with `adv_loss`'s shapes and returns: a "real" segment (True) has
    loss = -mean(logit) and dlogit = -scale / M, a "fake" one +mean(logit) and +scale / M."""
    _need_gpu(logit)
    return _adv_loss(logit, targets, _WASSERSTEIN, scale, want_grad)


def _adv_loss(logit, targets, mode, scale, want_grad, dlogit_out=None):
    N = logit.shape[0]
    if logit.numel() != N or logit.dtype != torch.float32 or N < 1:
        raise RuntimeError("adv_loss: float32 logits [N] or [N, 1, 1, 1] are expected")
    targets = [int(bool(t)) for t in targets]
    S = len(targets)
    if S < 1 or N % S != 0:
        raise RuntimeError(f"adv_loss: {N} logits do not split into {S} equal segments")
    out = torch.empty((2, S), device=logit.device, dtype=torch.float32)
    dlogit, lddl = None, 0
    if want_grad and dlogit_out is not None:
        if not (dlogit_out.is_cuda and dlogit_out.dtype == torch.float32 and dlogit_out.shape == (N, 1, 1, 1) and (N == 1 or dlogit_out.stride(0) == 4)):
            raise RuntimeError(f"adv_loss: dlogit_out is [{N}, 1, 1, 1] float32, a view of a [.., 1, 1, 4] buffer")
        dlogit, lddl = dlogit_out, 4
    elif want_grad and logit.dim() == 4:
        dlogit, lddl = torch.zeros((N, 1, 1, 4), device=logit.device, dtype=torch.float32)[..., :1], 4
    elif want_grad:
        dlogit, lddl = torch.empty(N, device=logit.device, dtype=torch.float32), 1
    check(load_library().mi_adv_loss(S, N // S, mode, (C.c_int * S)(*targets), float(scale), _p(logit), max(1, logit.stride(0)), _p(out[0]),
                                     _p(out[1]), _p(dlogit), lddl, _stream()), "mi_adv_loss")
    return out[0], out[1], dlogit


# --------------------------------------------------------------------------- InfoGAN heads and latent packing (info_head.hip)
INFO_HEAD_H = 128


def info_head_supported(S, M, E, Dd=0, V=0, Cc=0, H=INFO_HEAD_H) -> bool:
    """Dd = V = Cc = 0 asks about the D head alone."""
    return load_library().mi_info_head_supported(int(S), int(M), int(E), int(H), int(Dd), int(V), int(Cc)) == 1


def info_head_shape_ok(E) -> bool:
    """The feature widths mi_info_head_supported accepts, answered on the host (a module's constructor asks before any device exists)."""
    return E % 4 == 0 and 4 <= E <= 4096


def _info_rows(t, what, dtype=torch.float32):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
    if t.dim() != 2 or t.dtype != dtype or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{what}: {dtype} rows [N, width] with unit column stride")
    return t


def _info_ld(t):
    return max(t.shape[1], t.stride(0)) if t.shape[0] > 1 else t.shape[1]


def _info_ptrs(ts):
    """Six pointers w_d, b_d, W1, b1, W2, b2; None entries become null."""
    assert len(ts) == 6
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("info_head: parameters / gradients are dense float32 tensors on the HIP device")
    return (C.c_void_p * 6)(*[0 if t is None else t.data_ptr() for t in ts])


def info_latent(dis_c_index, cont_c, z, discrete_value):
    """The InfoGAN generator's NHWC input [N, 1, 1, latent_dim] (a view of a [N, 1, 1, ld] buffer, ld = latent_dim rounded up to 4,
    padded lanes 0) from dis_c_index [N, Dd] (int64), cont_c [N, Cc] and z [N, Nz]: ones at column v * Dd + d for v = dis_c_index[n, d],
    then the continuous codes, then the noise.  One launch.  An index outside [0, discrete_value) is not detected (that would need a
    host synchronisation): the columns of that code stay 0."""
    dis_c_index = _info_rows(dis_c_index, "dis_c_index", torch.int64)
    cont_c, z = _info_rows(cont_c, "cont_c"), _info_rows(z, "z")
    _need_gpu(cont_c)
    N, Dd = dis_c_index.shape
    Cc, Nz, V = cont_c.shape[1], z.shape[1], int(discrete_value)
    if cont_c.shape[0] != N or z.shape[0] != N or not dis_c_index.is_contiguous():
        raise RuntimeError(f"info_latent: dis_c_index (dense), cont_c and z with {N} rows each are expected")
    L = Dd * V + Cc + Nz
    ld = (L + 3) // 4 * 4
    out = torch.empty((N, 1, 1, ld), device=cont_c.device, dtype=torch.float32)
    check(load_library().mi_info_latent(N, Dd, V, Cc, Nz, _p(dis_c_index), _p(cont_c), _info_ld(cont_c), _p(z) if Nz else None,
                                        _info_ld(z) if Nz else 0, _p(out), ld, _stream()), "mi_info_latent")
    return out[..., :L]


def _info_feature(f):
    """f [rows, E] or the common layer's NHWC output [rows, 1, 1, E] (a view of a padded buffer: its pitch goes to the kernel)."""
    if not (torch.is_tensor(f) and f.is_cuda):
        raise RuntimeError("info_head: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
    _need_gpu(f)
    rows, E = f.shape[0], f.shape[-1]
    if f.dtype != torch.float32 or f.numel() != rows * E or (E > 1 and f.stride(-1) != 1):
        raise RuntimeError("info_head: float32 features [rows, E] or [rows, 1, 1, E] with unit column stride are expected")
    return rows, E, (max(E, f.stride(0)) if rows > 1 else E)


def info_head_fwd(f, params, targets, scale=1.0, codes=None, lambda_I=1.0):
    """The InfoGAN's D head, and with codes = (dis_c_index [rows, Dd] int64, cont_c [rows, Cc], discrete_value) its Q head and the
    mutual-information loss, on the shared feature f: LeakyReLU slope 0.01 (torch's default).  params: w_d [E], b_d [1], W1 [E, 128],
    b1 [128], W2 [128, Qd], b2 [Qd] (weights input-major; the last four may be None without codes).  targets: one bool per segment
    (1 or 2 equal segments of the rows).  Two launches.  Returns a record: logit [rows], loss [S] (binary cross-entropy with logits,
    per segment), mean_logit [S], dlogit = scale * d loss_s / d logit, and with codes q1 [rows, 128], q [rows, Qd] (column v * Dd + d
    is value v of code d), I_disc, I_cont and dq = lambda_I * d (I_disc + I_cont) / dq; the scalars are device tensors."""
    rows, E, ldf = _info_feature(f)
    targets = [int(bool(t)) for t in targets]
    S = len(targets)
    if S not in (1, 2) or rows % S != 0:
        raise RuntimeError(f"info_head_fwd: {rows} rows do not split into {S} equal segments (1 or 2)")
    M, dev, lib = rows // S, f.device, load_library()
    Dd = V = Cc = ldc = 0
    idx = cont = q1 = q = dq = None
    if codes is not None:
        idx, cont, V = _info_rows(codes[0], "dis_c_index", torch.int64), _info_rows(codes[1], "cont_c"), int(codes[2])
        Dd, Cc = idx.shape[1], cont.shape[1]
        if idx.shape[0] != rows or cont.shape[0] != rows or not idx.is_contiguous():
            raise RuntimeError(f"info_head_fwd: dis_c_index (dense) and cont_c with {rows} rows each are expected")
        ldc = _info_ld(cont)
    if lib.mi_info_head_supported(S, M, E, INFO_HEAD_H, Dd, V, Cc) != 1:
        check(-1, "mi_info_head_supported")
    if codes is not None:
        Qd = Dd * V + Cc
        q1 = torch.empty((rows, INFO_HEAD_H), device=dev, dtype=torch.float32)
        q, dq = (torch.empty((rows, Qd), device=dev, dtype=torch.float32) for _ in range(2))
    logit, dlogit = (torch.empty(rows, device=dev, dtype=torch.float32) for _ in range(2))
    ws = torch.empty(lib.mi_info_head_workspace_doubles(rows), device=dev, dtype=torch.float64)
    out6 = torch.empty(6, device=dev, dtype=torch.float32)
    check(lib.mi_info_head_fwd(S, M, E, INFO_HEAD_H, _p(f), ldf, _info_ptrs(params), targets[0], targets[-1], float(scale), Dd, V, Cc,
                               _p(idx), _p(cont), ldc, float(lambda_I), _p(logit), _p(dlogit), _p(q1), _p(q), _p(dq), _p(ws), _p(out6),
                               _stream()), "mi_info_head_fwd")
    return {"S": S, "M": M, "E": E, "f": f, "ldf": ldf, "logit": logit, "dlogit": dlogit, "q1": q1, "q": q, "dq": dq, "loss": out6[0:S],
            "mean_logit": out6[2:2 + S], "I_disc": out6[4], "I_cont": out6[5], "keep": (idx, cont)}


def info_q_fwd(f, params):
    """The Q head's output alone, q [rows, Qd] = LeakyReLU(LeakyReLU(f) W1 + b1) W2 + b2 (slope 0.01): one launch, no D head, no loss.
    params: W1 [E, 128], b1 [128], W2 [128, Qd], b2 [Qd], weights input-major."""
    rows, E, ldf = _info_feature(f)
    Qd, lib = params[2].shape[1], load_library()
    if lib.mi_info_head_supported(1, rows, E, INFO_HEAD_H, 0, 0, 0) != 1:
        check(-1, "mi_info_head_supported")
    q = torch.empty((rows, Qd), device=f.device, dtype=torch.float32)
    check(lib.mi_info_head_fwd(1, rows, E, INFO_HEAD_H, _p(f), ldf, _info_ptrs([None, None] + list(params)), 1, 1, 1.0, 0, 0, Qd, None, None, 0,
                               0.0, None, None, None, _p(q), None, None, None, _stream()), "mi_info_head_fwd")
    return q


def info_head_bwd(params, rec, grads=None, want_df=True, dlogit=None, q1=None, dq=None):
    """Backward of `info_head_fwd` from its record (dlogit / q1 / dq override the record's).  Returns df [rows, 1, 1, E], the feature
    gradient leaky'(f) (dlogit w_d + (leaky'(q1) (dq W2^T)) W1^T) in the shape ConvEncoder.backward_nhwc takes as dout, or None.
    grads: six tensors like params, None for what is not wanted -- the Q gradients (W1, b1, W2, b2) as a group, the D-head gradients
    (w_d, b_d) as a group; they are stored, not accumulated.  Two launches, one without parameter gradients."""
    S, M, E, f = rec["S"], rec["M"], rec["E"], rec["f"]
    rows, dev = S * M, f.device
    dlogit = rec["dlogit"] if dlogit is None else dlogit
    q1 = rec["q1"] if q1 is None else q1
    dq = rec["dq"] if dq is None else dq
    Qd = 0
    if dq is not None:
        Qd = dq.shape[1]
        if not (q1 is not None and q1.shape == (rows, INFO_HEAD_H) and q1.is_contiguous() and dq.shape[0] == rows and dq.is_contiguous()
                and q1.dtype == dq.dtype == torch.float32):
            raise RuntimeError("info_head_bwd: dense float32 q1 [rows, 128] and dq [rows, Qd] are expected")
    if dlogit.shape != (rows,) or not dlogit.is_contiguous() or dlogit.dtype != torch.float32:
        raise RuntimeError("info_head_bwd: dense float32 dlogit [rows] is expected")
    if grads is None and not want_df:
        raise RuntimeError("info_head_bwd: neither a feature gradient nor parameter gradients asked for")
    df = torch.empty((rows, 1, 1, E), device=dev, dtype=torch.float32) if want_df else None
    ws = None
    if grads is not None and grads[2] is not None:
        ws = torch.empty((rows, INFO_HEAD_H), device=dev, dtype=torch.float32)
    check(load_library().mi_info_head_bwd(S, M, E, INFO_HEAD_H, Qd, _p(f), rec["ldf"], _info_ptrs(params), _p(dlogit), _p(q1), _p(dq), _p(df),
                                          E, _p(ws), _info_ptrs(grads) if grads is not None else None, _stream()), "mi_info_head_bwd")
    return df


# --------------------------------------------------------------------------- AGE latent moments (age_ops.hip)
AGE_RECON = {None: 0, "none": 0, "cosine": 1, "mse": 2}
AGE_LMAX = 512


def age_moments_supported(S, M, L) -> bool:
    return load_library().mi_age_moments_supported(int(S), int(M), int(L)) == 1


def _age_rows(t, what):
    """t [rows, L] or an encoder's NHWC output [rows, 1, 1, L] (a view of a padded buffer: its pitch goes to the kernel)
    -> (rows, L, pitch)."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
    _need_gpu(t)
    rows, L = t.shape[0], t.shape[-1]
    if t.dtype != torch.float32 or t.dim() not in (2, 4) or t.numel() != rows * L or (L > 1 and t.stride(-1) != 1):
        raise RuntimeError(f"{what}: float32 rows [rows, L] or [rows, 1, 1, L] with unit column stride are expected")
    return rows, L, (max(L, t.stride(0)) if rows > 1 else L)


def age_moments_fwd(e, segments=1, normalize=True, stats=True, recon=(None, None), target=None):
    """The AGE's code statistics on e [S * M, L] (or the encoder's NHWC output [S * M, 1, 1, L], read in place): z = F.normalize(e) per
    row (normalize) or z = e; per segment mu [S, L], var [S, L] (unbiased), kl = mean(mu^2 + var - log var) / 2, mean(mu), mean(var);
    recon[s] "cosine" (1 - mean cosine similarity) or "mse" of the segment's z against target [M, L].  At most two launches.
    Returns a record for `age_moments_bwd`; z is dense [S * M, L] with normalize, else a [S * M, L] view of e; the scalars kl [S],
    mean_mu [S], mean_var [S], recon [S] are device tensors.  stats=False: the normalisation alone (one launch)."""
    rows, L, ld = _age_rows(e, "age_moments_fwd: e")
    S = int(segments)
    modes = [AGE_RECON[m] for m in (list(recon) + [None])[:2]]
    if S not in (1, 2) or rows % S != 0:
        raise RuntimeError(f"age_moments_fwd: {rows} rows do not split into {S} equal segments (1 or 2)")
    M, dev, lib = rows // S, e.device, load_library()
    if stats and lib.mi_age_moments_supported(S, M, L) != 1:
        check(-1, "mi_age_moments_supported")
    ldt = 0
    if any(modes):
        tr, tl, ldt = _age_rows(target, "age_moments_fwd: target")
        if (tr, tl) != (M, L):
            raise RuntimeError(f"age_moments_fwd: target [{M}, {L}] expected, got [{tr}, {tl}]")
    else:
        target = None
    z = norm = mu = var = out4 = ws = None
    if normalize:
        z = torch.empty((rows, L), device=dev, dtype=torch.float32)
        norm = torch.empty(rows, device=dev, dtype=torch.float32)
    if stats:
        mu, var = (torch.empty((S, L), device=dev, dtype=torch.float32) for _ in range(2))
        out4 = torch.empty((S, 4), device=dev, dtype=torch.float32)
        if any(modes):
            ws = torch.empty(lib.mi_age_moments_workspace_doubles(S, M), device=dev, dtype=torch.float64)
    check(lib.mi_age_moments_fwd(S, M, L, _p(e), ld, int(bool(normalize)), _p(z), _p(norm), int(bool(stats)), modes[0], modes[1],
                                 _p(target), ldt, _p(mu), _p(var), _p(out4), _p(ws), _stream()), "mi_age_moments_fwd")
    rec = {"S": S, "M": M, "L": L, "e": e, "z": z if normalize else torch.as_strided(e, (rows, L), (ld, 1)), "ldz": L if normalize else ld,
           "norm": norm, "mu": mu, "var": var, "modes": modes, "target": target, "ldt": ldt}
    if stats:
        rec.update(kl=out4[:, 0], mean_mu=out4[:, 1], mean_var=out4[:, 2], recon=out4[:, 3])
    return rec


def age_normalize(z):
    """F.normalize(z) for rows z [N, L]: one launch."""
    return age_moments_fwd(z, 1, normalize=True, stats=False)["z"]


def age_moments_bwd(rec, c, w=(0.0, 0.0), dz_ext=(None, None)):
    """Backward of `age_moments_fwd` from its record, one launch: per segment the KL coefficient c[s], the weight w[s] of the segment's
    reconstruction term and an optional external gradient dz_ext[s] by z ([M, L] or [M, 1, 1, L], any pitch) that is added.  Returns
    de [S * M, 1, 1, L], the gradient by e in the shape ConvEncoder.backward_nhwc takes as dout (a view of a [.., ld] buffer, ld = L
    rounded up to 4, whose padded lanes are 0)."""
    S, M, L = rec["S"], rec["M"], rec["L"]
    c, w, dz_ext = (list(c) + [0.0])[:2], (list(w) + [0.0])[:2], (list(dz_ext) + [None])[:2]
    if rec["mu"] is None:
        raise RuntimeError("age_moments_bwd: the record holds no statistics (stats=False)")
    ldx = 0
    for d in dz_ext:
        if d is not None:
            dr, dl, pitch = _age_rows(d, "age_moments_bwd: dz_ext")
            if (dr, dl) != (M, L) or (ldx and pitch != ldx):
                raise RuntimeError(f"age_moments_bwd: dz_ext [{M}, {L}] with one pitch expected")
            ldx = pitch
    ldde = (L + 3) // 4 * 4
    de = torch.empty((S * M, 1, 1, ldde), device=rec["z"].device, dtype=torch.float32)
    check(load_library().mi_age_moments_bwd(S, M, L, _p(rec["z"]), rec["ldz"], _p(rec["norm"]), _p(rec["mu"]), _p(rec["var"]), float(c[0]),
                                            float(c[1]), rec["modes"][0], rec["modes"][1], float(w[0]), float(w[1]), _p(rec["target"]),
                                            rec["ldt"], _p(dz_ext[0]), _p(dz_ext[1]), ldx, _p(de), ldde, _stream()), "mi_age_moments_bwd")
    return de[..., :L]


def age_image_mse(pred_nhwc, target_nchw, want_grad=True, gscale=1.0):
    """(F.mse_loss(pred, target), gscale * its gradient by pred) for pred NHWC [B, H, W, C] (a view of a padded buffer) and target NCHW:
    `eps_loss(..., 1)` with the loss summed in a fixed order instead of with an atomic, so that it has the same bits on every run.
    Two launches.  The gradient is a [B, H, W, C] view of a [.., ld] buffer whose padded lanes are 0."""
    _need_gpu(pred_nhwc)
    B, H, W, Cc = pred_nhwc.shape
    if not (torch.is_tensor(target_nchw) and target_nchw.is_cuda and target_nchw.dtype == torch.float32 and target_nchw.shape == (B, Cc, H, W)):
        raise RuntimeError(f"age_image_mse: a float32 target [{B}, {Cc}, {H}, {W}] on the HIP device is expected")
    target_nchw = target_nchw.contiguous()
    ld, dev, lib = ld_of(pred_nhwc), pred_nhwc.device, load_library()
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    dpred = torch.empty((B, H, W, ld), device=dev, dtype=torch.float32) if want_grad else None
    ws = torch.empty(lib.mi_age_image_mse_workspace_doubles(B, H * W), device=dev, dtype=torch.float64)
    check(lib.mi_age_image_mse(B, Cc, H * W, _p(pred_nhwc), ld, _p(target_nchw), _p(loss), _p(dpred), float(gscale), _p(ws), _stream()),
          "mi_age_image_mse")
    return loss[0], (dpred[..., :Cc] if want_grad else None)


# --------------------------------------------------------------------------- VAE-GAN operators (vaegan_ops.hip)
def _vg_rows(t, what, cols=None):
    """t [rows, cols] or a net's NHWC output [rows, 1, 1, cols] (a view of a padded buffer) -> (rows, cols, pitch)."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
    _need_gpu(t)
    rows, L = t.shape[0], t.shape[-1]
    if t.dtype != torch.float32 or t.dim() not in (2, 4) or t.numel() != rows * L or (L > 1 and t.stride(-1) != 1) or (cols and L != cols):
        raise RuntimeError(f"{what}: float32 rows [rows, {cols or 'L'}] or [rows, 1, 1, {cols or 'L'}] with unit column stride are expected")
    return rows, L, (max(L, t.stride(0)) if rows > 1 else L)


def vaegan_latent_fwd(h, eps, prior):
    """h [N, 2L] = [mu | log_sigma] (or the encoder's NHWC output [N, 1, 1, 2L], read in place), eps [N, L], prior [N, L] ->
    (zz [2N, 1, 1, L], kld): the decoder's NHWC input for ONE segments=2 pass, rows [0, N) = mu + exp(log_sigma) eps, rows [N, 2N) =
    prior -- a view of a [2N, 1, 1, 4 ceil(L / 4)] buffer whose padded lanes are 0 -- and the KL term of K.vae_latent_fwd, stored.
    One launch."""
    N, L2, ldh = _vg_rows(h, "vaegan_latent_fwd: h")
    L = L2 // 2
    if L2 != 2 * L or L < 1:
        raise RuntimeError("vaegan_latent_fwd: h holds [mu | log_sigma], an even number of columns")
    for t, what in ((eps, "eps"), (prior, "prior")):
        _vg_rows(t, f"vaegan_latent_fwd: {what}", L)
        if t.shape[0] != N or not t.is_contiguous():
            raise RuntimeError(f"vaegan_latent_fwd: {what} [{N}, {L}], dense, is expected")
    ldz = (L + 3) // 4 * 4
    lib = load_library()
    if lib.mi_vaegan_latent_supported(N, L) != 1:
        check(-1, "mi_vaegan_latent_supported")
    zz = torch.empty((2 * N, 1, 1, ldz), device=h.device, dtype=torch.float32)
    kld = torch.empty((), device=h.device, dtype=torch.float32)
    check(lib.mi_vaegan_latent_fwd(N, L, _p(h), ldh, _p(eps), _p(prior), _p(zz), ldz, _p(kld), _stream()), "mi_vaegan_latent_fwd")
    return zz[..., :L], kld


def vaegan_latent_bwd(h, eps, dz, g_kld=1.0, dz_scale=1.0):
    """dh [N, 1, 1, 2L] (a view of a [N, 1, 1, 4 ceil(2L / 4)] buffer whose padded lanes are 0: what ConvEncoder.backward_nhwc takes as
    dout) from the first N rows of dz (the decoder's input gradient [>= N, L] or [>= N, 1, 1, L], any pitch) times dz_scale, plus
    g_kld times the KL term's gradient.  One launch."""
    N, L2, ldh = _vg_rows(h, "vaegan_latent_bwd: h")
    L = L2 // 2
    rows, _, lddz = _vg_rows(dz, "vaegan_latent_bwd: dz", L)
    if rows < N or not (eps.is_cuda and eps.dtype == torch.float32 and eps.shape == (N, L) and eps.is_contiguous()):
        raise RuntimeError(f"vaegan_latent_bwd: dz with at least {N} rows and a dense float32 eps [{N}, {L}] on the device are expected")
    lddh = (L2 + 3) // 4 * 4
    dh = torch.empty((N, 1, 1, lddh), device=h.device, dtype=torch.float32)
    check(load_library().mi_vaegan_latent_bwd(N, L, _p(h), ldh, _p(eps), _p(dz), lddz, float(dz_scale), float(g_kld), _p(dh), lddh, _stream()),
          "mi_vaegan_latent_bwd")
    return dh[..., :L2]


def feat_match(real, recon, drecon=None, gscale=1.0, accumulate=False, want_grad=True):
    """The VAE-GAN's reconstruction loss in discriminator-feature space: (sum (real - recon)^2 / N, its gradient by recon times gscale)
    for two dense blocks [N, ...] of the same shape (two segments of netD's last hidden NHWC activation, read in place).  drecon: a
    dense block of that shape to store into, or to add into with accumulate (the recon segment's rows of netD's gradient buffer);
    None with want_grad allocates one; want_grad=False: the loss alone.  The loss is summed in a fixed order.  Two launches."""
    _need_gpu(real)
    N = real.shape[0]
    per = real[0].numel()
    if not (real.shape == recon.shape and real.dtype == recon.dtype == torch.float32 and real.is_contiguous() and recon.is_contiguous()):
        raise RuntimeError("feat_match: two dense float32 blocks of one shape are expected")
    if not want_grad:
        drecon = None
    elif drecon is None:
        if accumulate:
            raise RuntimeError("feat_match: accumulate needs the buffer to add into")
        drecon = torch.empty_like(recon)
    elif not (drecon.shape == recon.shape and drecon.dtype == torch.float32 and drecon.is_contiguous() and drecon.device == real.device):
        raise RuntimeError("feat_match: drecon is a dense float32 block shaped like recon")
    lib = load_library()
    if lib.mi_feat_match_supported(N, per) != 1:
        check(-1, "mi_feat_match_supported")
    loss = torch.empty(1, device=real.device, dtype=torch.float32)
    ws = torch.empty(lib.mi_feat_match_workspace_doubles(N, per), device=real.device, dtype=torch.float64)
    check(lib.mi_feat_match(N, per, _p(real), _p(recon), _p(loss), _p(drecon), float(gscale), int(bool(accumulate)), _p(ws), _stream()),
          "mi_feat_match")
    return loss[0], drecon


def vaegan_pack_fwd(dec_out, imgs):
    """netD's input for ONE segments=3 pass: [fake | nhwc(imgs) | recon] as [3N, H, W, C] (a view of a buffer with the decoder's pixel
    pitch, padded lanes 0) from the decoder's [recon | fake] NHWC output [2N, H, W, C] and the NCHW batch [N, C, H, W].  One launch."""
    _need_gpu(dec_out)
    N, Cc, H, W = imgs.shape
    if not (imgs.is_cuda and imgs.dtype == torch.float32 and imgs.is_contiguous() and dec_out.shape == (2 * N, H, W, Cc)):
        raise RuntimeError("vaegan_pack_fwd: a dense float32 batch [N, C, H, W] on the device and a decoder output [2N, H, W, C] are expected")
    ld = ld_of(dec_out)
    x = torch.empty((3 * N, H, W, ld), device=dec_out.device, dtype=torch.float32)
    check(load_library().mi_vaegan_pack_fwd(N, Cc, H * W, _p(dec_out), _p(imgs), _p(x), ld, _stream()), "mi_vaegan_pack_fwd")
    return x[..., :Cc]


def vaegan_unpack_bwd(dx, s_recon=1.0, s_fake=1.0):
    """The decoder's upstream gradient [s_recon dx[2N:3N] | s_fake dx[0:N]] as [2N, H, W, C] (padded lanes 0) from netD's input
    gradient dx [3N, H, W, C] over [fake | real | recon].  One launch."""
    _need_gpu(dx)
    N3, H, W, Cc = dx.shape
    if N3 % 3 != 0 or dx.dtype != torch.float32:
        raise RuntimeError("vaegan_unpack_bwd: a float32 gradient [3N, H, W, C] is expected")
    N, ld = N3 // 3, ld_of(dx)
    dy = torch.empty((2 * N, H, W, ld), device=dx.device, dtype=torch.float32)
    check(load_library().mi_vaegan_unpack_bwd(N, Cc, H * W, _p(dx), float(s_recon), float(s_fake), _p(dy), ld, _stream()), "mi_vaegan_unpack_bwd")
    return dy[..., :Cc]


# --------------------------------------------------------------------------- WGAN-GP operators (critic_ops.hip)
def _dense(*ts):
    for t in ts:
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32), "dense fp32 tensor expected"


def sample_norm_fwd(x, gamma, beta, eps=1e-5):
    """nn.GroupNorm(1, C) on a dense NHWC tensor -> (y, stats[N,2])."""
    _need_gpu(x); _dense(x)
    N, H, W, Cc = x.shape
    y = torch.empty_like(x)
    stats = torch.empty((N, 2), device=x.device, dtype=torch.float32)
    check(load_library().mi_sample_norm_fwd(N, H * W, Cc, _p(x), _p(gamma), _p(beta), _p(y), _p(stats), eps, _stream()), "mi_sample_norm_fwd")
    return y, stats


def sample_norm_bwd(x, stats, gamma, dy, dgamma=None, dbeta=None, extra=None, out=None):
    _dense(x, dy, extra, out)
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x) if out is None else out
    check(load_library().mi_sample_norm_bwd(N, H * W, Cc, _p(x), _p(stats), _p(gamma), _p(dy), _p(extra), _p(dx), _p(dgamma), _p(dbeta),
                                            _stream()), "mi_sample_norm_bwd")
    return dx


def sample_norm_bwd2(x, stats, gamma, dy, u, dgamma=None):
    """Backward of sample_norm_bwd: (adjoint wrt dy, adjoint wrt x); dgamma accumulated."""
    _dense(x, dy, u)
    N, H, W, Cc = x.shape
    adj_dy, adj_x = torch.empty_like(x), torch.empty_like(x)
    check(load_library().mi_sample_norm_bwd2(N, H * W, Cc, _p(x), _p(stats), _p(gamma), _p(dy), _p(u), _p(adj_dy), _p(adj_x), _p(dgamma),
                                             _stream()), "mi_sample_norm_bwd2")
    return adj_dy, adj_x


def leaky_relu_fwd(x, slope=0.2, inplace=False):
    _need_gpu(x); _dense(x)
    y = x if inplace else torch.empty_like(x)
    check(load_library().mi_leaky_relu_fwd(x.numel(), _p(x), _p(y), slope, _stream()), "mi_leaky_relu_fwd")
    return y


def leaky_relu_bwd(y, dy, slope=0.2, out=None):
    _dense(y, dy, out)
    dx = torch.empty_like(dy) if out is None else out
    check(load_library().mi_leaky_relu_bwd(y.numel(), _p(y), _p(dy), _p(dx), slope, _stream()), "mi_leaky_relu_bwd")
    return dx


def tanh_fwd(x, inplace=False):
    _need_gpu(x); _dense(x)
    y = x if inplace else torch.empty_like(x)
    check(load_library().mi_tanh_fwd(x.numel(), _p(x), _p(y), _stream()), "mi_tanh_fwd")
    return y


def tanh_bwd(y, dy, out=None):
    _dense(y, dy, out)
    dx = torch.empty_like(dy) if out is None else out
    check(load_library().mi_tanh_bwd(y.numel(), _p(y), _p(dy), _p(dx), _stream()), "mi_tanh_bwd")
    return dx


def lerp_rows(a, b, e):
    """e[s] * a[s] + (1 - e[s]) * b[s] over the leading dimension."""
    _need_gpu(a); _dense(a, b)
    out = torch.empty_like(a)
    check(load_library().mi_lerp_rows(a.shape[0], a[0].numel(), _p(a), _p(b), _p(e), _p(out), _stream()), "mi_lerp_rows")
    return out


def gp_penalty(g, want_grad=True, scale=1.0, scale_dev=None):
    """(mean_s (||g_s|| - 1)^2, scale * d penalty / d g) for a dense [N, ...] gradient tensor."""
    _need_gpu(g); _dense(g)
    pen = torch.zeros((), device=g.device, dtype=torch.float32)
    u = torch.empty_like(g) if want_grad else None
    check(load_library().mi_gp_penalty(g.shape[0], g[0].numel(), _p(g), _p(pen), _p(u), scale, _p(scale_dev), _stream()), "mi_gp_penalty")
    return pen, u


def nchw_to_nhwc(x, ld=None):
    _need_gpu(x)
    B, Cc, H, W = x.shape
    ld = ld or (Cc + 3) // 4 * 4
    x = x.contiguous()
    y = torch.empty((B, H, W, ld), device=x.device, dtype=torch.float32)
    check(load_library().mi_nchw_to_nhwc(B, Cc, H * W, _p(x), _p(y), ld, _stream()), "mi_nchw_to_nhwc")
    return y[..., :Cc]


def nhwc_to_nchw(x):
    B, H, W, Cc = x.shape
    y = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
    check(load_library().mi_nhwc_to_nchw(B, Cc, H * W, _p(x), ld_of(x), _p(y), _stream()), "mi_nhwc_to_nchw")
    return y


def q_sample(x0, noise, t, sqrt_ac, sqrt_1mac, want_nchw=False):
    _need_gpu(x0)
    B, Cc, H, W = x0.shape
    ld = (Cc + 3) // 4 * 4
    x0 = x0.contiguous(); noise = noise.contiguous()
    xt = torch.empty((B, H, W, ld), device=x0.device, dtype=torch.float32)
    xt_nchw = torch.empty_like(x0) if want_nchw else None
    check(load_library().mi_q_sample(B, Cc, H * W, _p(x0), _p(noise), _p(t), _p(sqrt_ac), _p(sqrt_1mac), _p(xt), ld,
                                     _p(xt_nchw), _stream()), "mi_q_sample")
    return xt[..., :Cc], xt_nchw


def eps_loss(pred_nhwc, target_nchw, loss_type=0, want_grad=True, gscale=1.0):
    B, H, W, Cc = pred_nhwc.shape
    target_nchw = target_nchw.contiguous()
    loss = torch.zeros((), device=pred_nhwc.device, dtype=torch.float32)
    ld = ld_of(pred_nhwc)
    dpred = torch.empty((B, H, W, ld), device=pred_nhwc.device, dtype=torch.float32) if want_grad else None
    check(load_library().mi_eps_loss(B, Cc, H * W, _p(pred_nhwc), ld, _p(target_nchw), loss_type, _p(loss), _p(dpred),
                                     gscale, _stream()), "mi_eps_loss")
    return loss, (dpred[..., :Cc] if want_grad else None)


def p_sample_update(x, eps_nhwc, z, t, tab, clip=True, want_nhwc=True, out=None, out_nhwc=None):
    """x_{t-1} from (x_t, eps prediction, z).  out: where the NCHW result goes (may be x itself: in place); out_nhwc: a [B, H, W, ldo]
    buffer (padding channels zero) that receives the NHWC copy -- the graph sampler's static buffers."""
    B, Cc, H, W = x.shape
    ldo = (Cc + 3) // 4 * 4
    xp = torch.empty_like(x) if out is None else out
    if out_nhwc is not None:
        assert out_nhwc.shape == (B, H, W, ldo) and out_nhwc.is_contiguous() and out_nhwc.dtype == torch.float32
        xp_nhwc = out_nhwc
    else:
        xp_nhwc = torch.zeros((B, H, W, ldo), device=x.device, dtype=torch.float32) if want_nhwc else None
    check(load_library().mi_p_sample_update(
        B, Cc, H * W, _p(x), _p(eps_nhwc), ld_of(eps_nhwc), _p(z), _p(t), _p(tab["sqrt_recip_alphas_cumprod"]),
        _p(tab["sqrt_recipm1_alphas_cumprod"]), _p(tab["posterior_mean_coef1"]), _p(tab["posterior_mean_coef2"]),
        _p(tab["posterior_log_variance_clipped"]), int(clip), _p(xp), _p(xp_nhwc), ldo, _stream()), "mi_p_sample_update")
    return xp, (xp_nhwc[..., :Cc] if want_nhwc else None)


def adam_step(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0, host_complements=False):
    """host_complements: 1 - b1 and 1 - b2 are formed here in double and rounded once (mi_adam_step_c), as torch's scalars are; the
    default forms them in fp32 on the device, where 1.f - 0.999f is off by 4.7e-5."""
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    e0 = _probe_open()
    if host_complements:
        check(load_library().mi_adam_step_c(p.numel(), _p(p), _p(g), _p(m), _p(v), lr, b2, 1.0 - b1, 1.0 - b2, eps, bc1, bc2, gscale,
                                            _stream()), "mi_adam_step_c")
    else:
        check(load_library().mi_adam_step(p.numel(), _p(p), _p(g), _p(m), _p(v), lr, b1, b2, eps, bc1, bc2, gscale, _stream()),
              "mi_adam_step")
    if e0 is not None:
        _probe_close(e0, "adam_kernel", 0.0, f"{p.numel()} params", p.numel() * 28.0)


def adam_tick(state):
    check(load_library().mi_adam_tick(_p(state), _stream()), "mi_adam_tick")


def adam_step_dev(p, g, m, v, state, b1, b2, eps, gscale=1.0):
    """Adam with step count / learning rate in `state` (device float[2]): graph-capturable."""
    check(load_library().mi_adam_step_dev(p.numel(), _p(p), _p(g), _p(m), _p(v), _p(state), b1, b2, eps, gscale, _stream()), "mi_adam_step_dev")


def rmsprop_step(p, g, v, lr, alpha=0.99, eps=1e-8, gscale=1.0):
    """torch.optim.RMSprop's default update (no momentum, not centered, no weight decay) of the flat buffer p from g, in one launch."""
    _need_gpu(p); _dense(p, g, v)
    if not (p.numel() == g.numel() == v.numel()):
        raise RuntimeError("rmsprop_step: p, g and v differ in size")
    check(load_library().mi_rmsprop_step(p.numel(), _p(p), _p(g), _p(v), lr, alpha, eps, gscale, _stream()), "mi_rmsprop_step")


def clamp_(p, lo, hi):
    """torch.clamp_(p, lo, hi) on a dense fp32 tensor in one launch: NaN stays NaN, -0.0 stays -0.0."""
    _need_gpu(p); _dense(p)
    check(load_library().mi_clamp_inplace(p.numel(), _p(p), float(lo), float(hi), _stream()), "mi_clamp_inplace")
    return p


def axpby(a, x, y, accumulate):
    """y = a*x (+ y).  x, y: same logical shape; strided channel slices allowed for 4-D."""
    if x.is_contiguous() and y.is_contiguous():
        check(load_library().mi_axpby(x.numel(), a, _p(x), int(accumulate), _p(y), _stream()), "mi_axpby")
    else:
        Cc = x.shape[-1]
        M = x.shape[0] * x.shape[1] * x.shape[2] if x.dim() == 4 else x.shape[0]
        check(load_library().mi_axpby2d(M, Cc, a, _p(x), ld_of(x), int(accumulate), _p(y), ld_of(y), _stream()), "mi_axpby2d")


def scale_by_device_scalar(x, s):
    """x *= s where s is a 0-d/1-element fp32 tensor on the device."""
    s = s.reshape(1).float()
    check(load_library().mi_scale_by_device_scalar(_rows(x), x.shape[-1], _p(x), ld_of(x), _p(s), _stream()),
          "mi_scale_by_device_scalar")


def gather_rows(table, idx):
    """table[T, C] fp32, idx int64 [B] on the device -> [B, C]."""
    out = torch.empty((idx.shape[0], table.shape[1]), device=table.device, dtype=torch.float32)
    check(load_library().mi_gather_rows(idx.shape[0], table.shape[1], _p(table), _p(idx), _p(out), _stream()), "mi_gather_rows")
    return out


def clock_probe(device, usec=300, blocks=256):
    """Shader clock (MHz) workgroup 0 sustained while `blocks` workgroups issue back-to-back bf16 MFMAs for `usec` microseconds
    (mi_debug_clock_probe: s_memtime ticks over 100 MHz wall-clock ticks).  A measurement aid for bench.py; synchronises."""
    out = torch.zeros(3, device=device, dtype=torch.int64)
    check(load_library().mi_debug_clock_probe(blocks, usec, _p(out), _stream()), "mi_debug_clock_probe")
    torch.cuda.synchronize()
    s, w = int(out[0]), int(out[1])
    return round(100.0 * s / max(w, 1), 1)


def u8_gather_normalize(data_u8, idx, flip=None, normalize=True):
    """data_u8: uint8 [N,H,W,C] on the device, idx: int64 [B], flip: uint8/bool [B] or None -> fp32 NCHW batch [B,C,H,W] with the
    reference transform chain applied (ToTensor, flip, Normalize(0.5, 0.5))."""
    if not data_u8.is_cuda or data_u8.dtype != torch.uint8 or not data_u8.is_contiguous():
        raise RuntimeError("u8_gather_normalize needs a contiguous uint8 dataset tensor on the HIP device")
    if data_u8.device.index != torch.cuda.current_device():
        raise RuntimeError("dataset tensor is not on the current HIP device")
    N, H, W, Cc = data_u8.shape
    idx = idx.to(device=data_u8.device, dtype=torch.int64).contiguous()
    if flip is not None:
        flip = flip.to(device=data_u8.device, dtype=torch.uint8).contiguous()
    out = torch.empty((idx.shape[0], Cc, H, W), device=data_u8.device, dtype=torch.float32)
    check(load_library().mi_u8_gather_normalize(idx.shape[0], Cc, H, W, _p(data_u8), _p(idx), _p(flip), int(normalize), _p(out), _stream()),
          "mi_u8_gather_normalize")
    return out


@_cached_question
def fast3x3_supported(N, H, W, K, Nc, K1=None):
    """(conv via the LDS-tile kernel?, wgrad via the image-major kernel?) for a 3x3/s1/p1 layer in bf16 mode."""
    lib = load_library()
    dc = _conv_desc(N, H, W, K, Nc, 3, K1=K1 or K, ldx=4, ldx2=4)
    dw = _wgrad_desc(N, (H, W), (H, W), K, Nc, 3, 1, 1, True, MODE_BF16, 4, 4, I1=K1 or K, ldp2=4)
    return bool(lib.mi_conv3x3_bf16w_supported(C.byref(dc))), bool(lib.mi_conv3x3_wgrad_supported(C.byref(dw)))


@_cached_question
def fast1x1_supported(N, H, W, K, Nc):
    """(conv + dgrad via the LDS-tile kernel?, wgrad via the image-major kernel?) for a 1x1 layer in bf16 mode."""
    lib = load_library()
    ok = all(lib.mi_conv3x3_bf16w_supported(C.byref(_conv_desc(N, H, W, k, n, 1, ldx=8, ldx2=8))) for k, n in ((K, Nc), (Nc, K)))   # forward, dgrad
    dw = _wgrad_desc(N, (H, W), (H, W), K, Nc, 1, 1, 0, True, MODE_BF16, 8, 8, ldp2=8)
    return ok, bool(lib.mi_conv3x3_wgrad_supported(C.byref(dw)))


@_cached_question
def conv1x1_tile_supported(N, H, W, K, Nc, K1=None):
    """Does the 1x1 tile kernel take the forward conv over dense bf16 input(s) -- K1 < K: the skip concat's two sources, K1 and K - K1
    channels (res_conv of the up path)?  conv3x3_bf16w(ksize=1) then returns a tensor."""
    k1 = K1 or K
    return bool(_query("mi_conv3x3_bf16w_supported", _conv_desc(N, H, W, K, Nc, 1, K1=k1, ldx=k1, ldx2=(K - k1) if k1 < K else 0)))


@_cached_question
def conv3x3_uses_splitk(N, H, W, K, Nc, K1=None):
    """Would the 3x3 LDS-tile kernel run this layer with the split-K plan (fp32 output only)?"""
    return bool(_query("mi_conv3x3_bf16w_uses_splitk", _conv_desc(N, H, W, K, Nc, 3, K1=K1 or K, ldx=4, ldx2=4)))


# ---------------------------------------------------------------------------------------------------------- PixelCNN (csrc/pixelcnn.hip)
PCNN_PLAIN, PCNN_GATE_TS, PCNN_GATE_TT, PCNN_ELU_GRAD = 0, 1, 2, 3


def _ld(t):
    """pixel pitch of an NHWC activation (a channel slice of a contiguous tensor is legal)"""
    if t.is_contiguous():                      # size-1 dimensions may carry any stride
        return t.shape[3]
    assert t.dim() == 4 and t.stride(3) == 1 and t.stride(1) == t.shape[2] * t.stride(2) and t.stride(0) == t.shape[1] * t.stride(1), \
        "NHWC activation with dense pixels expected"
    return t.stride(2)


def pcnn_desc(N, H, W, Cin, ldx, Cout, taps, w_strides, C2=0, ldx2=0, w2_strides=(0, 0), epi=PCNN_PLAIN, elu_in=False, accumulate=False,
              gate_C=0, ldy=0, ldpre=0, ldcond=0, ldr=0, ldaux=0, mode=MODE_FP32):
    """taps: [(dy, dx, tap index into the weight)]; w_strides = (w_sk, w_sc) -- see mi_pcnn_conv in include/mi_ddpm.h."""
    from .lib import MiPcnnConvDesc
    d = MiPcnnConvDesc(N=N, H=H, W=W, Cin=Cin, ldx=ldx, Cout=Cout, ldy=ldy, ntaps=len(taps), w_sk=w_strides[0], w_sc=w_strides[1],
                       C2=C2, ldx2=ldx2, w2_sk=w2_strides[0], w2_sc=w2_strides[1], epi=epi, elu_in=int(elu_in), accumulate=int(accumulate),
                       gate_C=gate_C, ldpre=ldpre, ldcond=ldcond, ldr=ldr, ldaux=ldaux, mode=mode)
    for i, (a, b, t) in enumerate(taps):
        d.tap_dy[i], d.tap_dx[i], d.tap_w[i] = a, b, t
    return d


def pcnn_conv(x, w, taps, w_strides, Cout, bias=None, x2=None, w2=None, w2_strides=(0, 0), bias2=None, epi=PCNN_PLAIN, cond=None,
              res=None, aux=None, out=None, pre=None, accumulate=False, elu_in=False, mode=MODE_FP32):
    """Masked dilated conv over the live taps (mi_pcnn_conv); mode MODE_FP32 / MODE_BF16 (matrix-core operands).  x [N,H,W,Cin] NHWC; gated epilogues return (y [.., Cout/2], pre [.., Cout])."""
    _need_gpu(x)
    N, H, W, Cin = x.shape
    gated = epi in (PCNN_GATE_TS, PCNN_GATE_TT)
    gC = Cout // 2 if gated else 0
    if out is None:
        out = torch.empty((N, H, W, gC if gated else Cout), device=x.device)
    if gated and pre is None:
        pre = torch.empty((N, H, W, Cout), device=x.device)
    d = pcnn_desc(N, H, W, Cin, _ld(x), Cout, taps, w_strides, C2=0 if x2 is None else x2.shape[3], ldx2=0 if x2 is None else _ld(x2),
                  w2_strides=w2_strides, epi=epi, elu_in=elu_in, accumulate=accumulate, gate_C=gC, ldy=_ld(out),
                  ldpre=0 if pre is None else _ld(pre), ldcond=0 if cond is None else cond.stride(0), ldr=0 if res is None else _ld(res),
                  ldaux=0 if aux is None else _ld(aux), mode=mode)
    check(load_library().mi_pcnn_conv(C.byref(d), _p(x), _p(w), _p(bias), _p(x2), _p(w2), _p(bias2), _p(cond), _p(res), _p(aux), _p(out),
                                       _p(pre), _stream()), "mi_pcnn_conv")
    return (out, pre) if gated else out


def pcnn_wgrad(x, dy, dw, taps, w_strides, elu_in=False, mode=MODE_FP32):
    """dw[c*w_sk + o*w_sc + tap] += sum_p x[p + off][c] dy[p][o] over the live taps (mi_pcnn_wgrad); dw flat fp32 storage."""
    _need_gpu(x)
    N, H, W, Cin = x.shape
    d = pcnn_desc(N, H, W, Cin, _ld(x), dy.shape[3], taps, w_strides, elu_in=elu_in, mode=mode)
    check(load_library().mi_pcnn_wgrad(C.byref(d), _p(x), _p(dy), _ld(dy), _p(dw), _stream()), "mi_pcnn_wgrad")


def pcnn_colsum(g, out, out2=None):
    M = g.shape[0] * g.shape[1] * g.shape[2]
    check(load_library().mi_pcnn_colsum(M, g.shape[3], _p(g), _ld(g), _p(out), _p(out2), _stream()), "mi_pcnn_colsum")


def pcnn_gate_bwd(pre, dout, kind, cond=None, dcond=None, dpre=None):
    """d pre of a gate (mi_pcnn_gate_bwd); cond / dcond: [N, >= 2C] row views (dcond accumulated)."""
    N, H, W, C2 = pre.shape
    Cg = C2 // 2
    if dpre is None:
        dpre = torch.empty_like(pre)
    ldc = cond.stride(0) if cond is not None else (dcond.stride(0) if dcond is not None else 0)
    if cond is not None and dcond is not None:
        assert cond.stride(0) == dcond.stride(0)
    check(load_library().mi_pcnn_gate_bwd(N, H * W, Cg, kind, _p(pre), _ld(pre), _p(cond), ldc, _p(dout), _ld(dout), _p(dpre), _ld(dpre),
                                           _p(dcond), _stream()), "mi_pcnn_gate_bwd")
    return dpre


def pcnn_small_mm(I, J, Kd, A, sai, sak, B, sbk, sbj, out, ldo, accumulate=False):
    check(load_library().mi_pcnn_small_mm(I, J, Kd, _p(A), sai, sak, _p(B), sbk, sbj, _p(out), ldo, int(accumulate), _stream()),
          "mi_pcnn_small_mm")


def pcnn_cond_rows(labels, w, out):
    """out[n][j] = w[j][labels[n]] (mi_pcnn_cond_rows); labels int64 [N], w [J, ncls]."""
    J, ncls = w.shape
    check(load_library().mi_pcnn_cond_rows(labels.shape[0], J, ncls, _p(labels), _p(w), _p(out), out.stride(0), _stream()), "mi_pcnn_cond_rows")
    return out


def pcnn_cond_wgrad(labels, dcond, dw):
    """dw[j][labels[n]] += dcond[n][j] (mi_pcnn_cond_wgrad)."""
    J, ncls = dw.shape
    check(load_library().mi_pcnn_cond_wgrad(labels.shape[0], J, ncls, _p(labels), _p(dcond), dcond.stride(0), _p(dw), _stream()),
          "mi_pcnn_cond_wgrad")


def pcnn_head_fwd(h, w, b, img, normalize, lse=None, partial=None, loss=None):
    """Fused ELU -> 1x1 -> log-sum-exp -> NLL -> bits per dim (mi_pcnn_head_fwd).  Returns (loss [1], lse)."""
    _need_gpu(h)
    N, H, W, Ch = h.shape
    Cc = img.shape[1]
    lib = load_library()
    if lse is None:
        lse = torch.empty(N * H * W * Cc, device=h.device)
    if partial is None:
        partial = torch.empty(lib.mi_pcnn_head_partials(N, H * W, Cc), device=h.device)
    if loss is None:
        loss = torch.empty(1, device=h.device)
    check(lib.mi_pcnn_head_fwd(N, Cc, H * W, Ch, _p(h), _ld(h), _p(w), _p(b), _p(img), int(normalize), _p(lse), _p(partial), _p(loss),
                               _stream()), "mi_pcnn_head_fwd")
    return loss, lse


def pcnn_head_dlogits(h, w, b, img, normalize, lse, gscale=None, out=None):
    """dlogits [N,H,W,256*Cc] = (softmax - onehot) * (*gscale) / (N*C*H*W*ln 2) (mi_pcnn_head_dlogits)."""
    N, H, W, Ch = h.shape
    Cc = img.shape[1]
    if out is None:
        out = torch.empty((N, H, W, 256 * Cc), device=h.device)
    check(load_library().mi_pcnn_head_dlogits(N, Cc, H * W, Ch, _p(h), _ld(h), _p(w), _p(b), _p(img), int(normalize), _p(lse), _p(gscale),
                                               _p(out), _stream()), "mi_pcnn_head_dlogits")
    return out


def pcnn_sample_step(h, w, b, counter, uniforms, img, xin, normalize):
    """One inverse-CDF pixel step at *counter (mi_pcnn_sample_step); img NCHW and xin NHWC are written in place."""
    N, Cc, H, W = img.shape
    check(load_library().mi_pcnn_sample_step(N, Cc, H, W, h.shape[3], _p(h), _ld(h), _p(w), _p(b), _p(counter), _p(uniforms), _p(img),
                                              _p(xin), _ld(xin), int(normalize), _stream()), "mi_pcnn_sample_step")


def pcnn_zero(t):
    check(load_library().mi_pcnn_zero(_p(t), t.numel() * t.element_size(), _stream()), "mi_pcnn_zero")


# ---------------------------------------------------------------------------------------------------------- MADE (csrc/made.hip)
def made_linear(x, w, b, deg_in, deg_out, act, out=None, mode=MODE_FP32):
    """y = act(x (W .* M)^T + b), M[o][i] = deg_out[o] >= deg_in[i] (mi_made_linear); act: sigmoid when True.  x [N, in] rows."""
    _need_gpu(x)
    N, fin = x.shape
    fout = w.shape[0]
    if out is None:
        out = torch.empty((N, fout), device=x.device)
    check(load_library().mi_made_linear(mode, N, fin, fout, _p(x), x.stride(0), _p(w), _p(b), _p(deg_in), _p(deg_out), int(act), _p(out),
                                        out.stride(0), _stream()), "mi_made_linear")
    return out


def made_dgrad(gy, w, deg_in, deg_out, s_in=None, out=None, work=None, mode=MODE_FP32):
    """dx = (gy (W .* M)) * s_in (1 - s_in) (mi_made_dgrad; s_in None: no factor).  gy [N, out]."""
    N, fout = gy.shape
    fin = w.shape[1]
    lib = load_library()
    if out is None:
        out = torch.empty((N, fin), device=gy.device)
    if work is None:
        work = torch.empty(lib.mi_made_dgrad_workspace(N, fin, fout) // 4, device=gy.device)
    check(lib.mi_made_dgrad(mode, N, fin, fout, _p(gy), gy.stride(0), _p(w), _p(deg_in), _p(deg_out), _p(s_in),
                            0 if s_in is None else s_in.stride(0), _p(work), _p(out), out.stride(0), _stream()), "mi_made_dgrad")
    return out


def made_dgrad_workspace(N, fin, fout):
    return load_library().mi_made_dgrad_workspace(N, fin, fout) // 4


def made_wgrad(gy, x, deg_in, deg_out, dw, db, mode=MODE_FP32):
    """dW[o][i] = sum_n gy[n][o] x[n][i] on the live entries only, db = column sums of gy (mi_made_wgrad); both written."""
    N, fout = gy.shape
    fin = x.shape[1]
    check(load_library().mi_made_wgrad(mode, N, fin, fout, _p(gy), gy.stride(0), _p(x), x.stride(0), _p(deg_in), _p(deg_out), _p(dw), _p(db),
                                       _stream()), "mi_made_wgrad")


def made_head_fwd(h, w, b, deg_in, deg_out, img, normalize, lse=None, partial=None, loss=None, mode=MODE_FP32):
    """Fused head -> log-sum-exp -> NLL -> bits per dim (mi_made_head_fwd); img [N, D] (any shape with N rows).  Returns (loss [1], lse [N, D])."""
    _need_gpu(h)
    N, Hd = h.shape
    D = w.shape[0] // 256
    lib = load_library()
    if lse is None:
        lse = torch.empty((N, D), device=h.device)
    if partial is None:
        partial = torch.empty(lib.mi_made_head_partials(N, D), device=h.device)
    if loss is None:
        loss = torch.empty(1, device=h.device)
    check(lib.mi_made_head_fwd(mode, N, D, Hd, _p(h), h.stride(0), _p(w), _p(b), _p(deg_in), _p(deg_out), _p(img), int(normalize), _p(lse),
                               _p(partial), _p(loss), _stream()), "mi_made_head_fwd")
    return loss, lse


def made_head_dlogits(h, w, b, deg_in, deg_out, img, normalize, lse, gscale=None, out=None, mode=MODE_FP32):
    """dlogits [N, 256 D] = (softmax - onehot) * (*gscale) / (N D ln 2), recomputed from lse (mi_made_head_dlogits)."""
    N, Hd = h.shape
    D = w.shape[0] // 256
    if out is None:
        out = torch.empty((N, 256 * D), device=h.device)
    check(load_library().mi_made_head_dlogits(mode, N, D, Hd, _p(h), h.stride(0), _p(w), _p(b), _p(deg_in), _p(deg_out), _p(img),
                                              int(normalize), _p(lse), _p(gscale), _p(out), _stream()), "mi_made_head_dlogits")
    return out


def made_head_rows(h, w, b, deg_in, deg_out, pos, C, HW, out, mode=MODE_FP32):
    """logits [N, 256 C] of the C units at raster position *pos (mi_made_head_rows)."""
    N, Hd = h.shape
    check(load_library().mi_made_head_rows(mode, N, C, HW, Hd, _p(h), h.stride(0), _p(w), _p(b), _p(deg_in), _p(deg_out), _p(pos), _p(out),
                                           _stream()), "mi_made_head_rows")
    return out


def made_sample_step(logits, counter, uniforms, img, normalize):
    """One inverse-CDF step at position *counter (mi_made_sample_step); img [N, C, H, W] written in place."""
    N, Cc, H, W = img.shape
    check(load_library().mi_made_sample_step(N, Cc, H * W, _p(logits), _p(counter), _p(uniforms), _p(img), int(normalize), _stream()),
          "mi_made_sample_step")
