/*
 * mi_ddpm.h -- C ABI of the MI355X (gfx950) DDPM hot-path library (libmi_ddpm.so).
 *
 * The reference (Victarry/Image-Generation-models) has NO FFI or plugin interface: its
 * hot path is Python calling stock ATen ops.  This header is
 * therefore the boundary a maintainer would bind from src/models/ddpm.py (ctypes stub in
 * INTEGRATION.md); every entry point cites the reference lines it replaces
 * (paths relative to /root/reference/).
 *
 * Contract
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator);
 *    the library never allocates, frees, retains or synchronises -> hipGraph-capture safe.
 *  - `stream` is a hipStream_t passed as void*; work is ordered only by that stream.
 *  - return 0 on success, <0 argument/shape error, >0 a hipError_t; mi_last_error() gives
 *    the thread-local message.  Nothing throws across the boundary.
 *  - activations are fp32 NHWC ("pixel-major"): element (n,y,x,c) at ((n*H+y)*W+x)*ld + c,
 *    ld >= C, ld % 4 == 0, base 16-byte aligned.
 *  - convolution weights live in tap-major layout  w[ky][kx][Cin][Cout]  (a permuted VIEW of
 *    the PyTorch [Cout,Cin,kh,kw] / ConvTranspose [Cin,Cout,kh,kw] parameter, see
 *    image-generation-models_amd/src/models/ddpm.py) so forward, dgrad, wgrad and the
 *    optimizer all stream the same contiguous buffer with no repack.
 *  - `mode`: 0 = exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = bf16 MFMA with fp32
 *    accumulate (v_mfma_f32_32x32x16_bf16; operands rounded to bf16 when staged to LDS).
 */
#ifndef MI_DDPM_H
#define MI_DDPM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ABI_VERSION 4   /* 2: mi_pack_weights_bf16 takes the fragment-order copies; mi_adam_step_dev betas are double.  3: mi_conv1x1_pw takes x2.  4: GroupNorm epilogue sums are 64-bit fixed point */
#define MI_MODE_FP32 0
#define MI_MODE_BF16 1

int mi_abi_version(void);
const char* mi_last_error(void);

/* ---- implicit-GEMM convolution on MFMA ---------------------------------------------
 * One kernel family for nn.Conv2d k3/k1 (ddpm.py:116,134,151-152,236), stride-2
 * Downsample (ddpm.py:79), ConvTranspose2d k4 s2 (ddpm.py:70), every data-gradient of
 * those (aten::convolution_backward) and nn.Linear (ddpm.py:127,190-192; H=W=1).
 *   y[n,oy,ox,j] (+)= bias[j] + residual[n,oy,ox,j]
 *                     + sum_{ky,kx,k} src[n,iy,ix,k] * W(ky,kx,k,j)
 *   transposed=0: iy = oy*stride - pad + ky          (convolution forward)
 *   transposed=1: iy = (oy + pad - ky)/stride, only where divisible (transposed conv / dgrad)
 *   src channel k comes from x when k < K1, else from x2 at k-K1 (skip concat ddpm.py:255
 *   without materialising the cat).
 *   W(ky,kx,k,j) = w[((ky*KW+kx)*K + k)*Nc + j] if w_kn else w[((ky*KW+kx)*Nc + j)*K + k].
 */
typedef struct MiConvDesc {
    int N;               /* batch */
    int IH, IW;          /* spatial size of the gathered tensor */
    int OH, OW;          /* spatial size of the produced tensor */
    int K;               /* contraction channels */
    int Nc;              /* produced channels */
    int KH, KW, stride, pad;
    int transposed;
    int w_kn;
    int mode;
    int K1;              /* channels taken from x; K1 == K -> single source */
    int ldx, ldx2, ldy, ldr;
    int accumulate;      /* y += result instead of y = result */
} MiConvDesc;

int mi_conv_igemm(const MiConvDesc* d, const float* x, const float* x2, const float* w,
                  const float* bias, const float* residual, float* y, void* stream);

/* same contract with the bf16 weight copy [tap][Nc][K] of mi_pack_weights_bf16 (mode 1, K % 8 == 0);
 * used for the stride-2 / transposed convolutions */
int mi_conv_igemm_bf16w(const MiConvDesc* d, const float* x, const float* x2, const void* w_nk_bf16,
                        const float* bias, const float* residual, float* y, void* stream);
/* ... with bf16-STORED activations (x_is_bf16 != 0: x / x2 are bf16 tensors, strides in elements and % 8 == 0, K and K1 % 64 == 0):
 * the Downsample conv, the Upsample transposed conv and their data gradients (ddpm.py:70,79) read the bf16 copies that the
 * skip connection / the weight gradient already have -- a 16-byte load is 8 channels, so a ring stage covers 64 channels (half the
 * barriers per MFMA, half the bytes, no pack).  Only layers the ring kernel takes; query _supported first.  y stays fp32. */
int mi_conv_igemm_bf16w_io_supported(const MiConvDesc* d);
int mi_conv_igemm_bf16w_io(const MiConvDesc* d, const void* x, const void* x2, const void* w_nk_bf16,
                           const float* bias, const float* residual, float* y, int x_is_bf16, void* stream);
/* tile instantiation mi_conv_igemm will launch for d (BM x BN); used to attribute profiles */
int mi_conv_igemm_tile(const MiConvDesc* d, int* bm, int* bn);
/* What the dispatch behind mi_conv_igemm / _bf16w / _bf16w_io decides for d (read-only; the dispatch launches from the same function).
 * has_wb: the bf16 weight copy is given; in16: bf16-stored activations; aligned: x, x2 are 16-byte aligned (the pitches are read from d).
 * Returns non-zero with mi_last_error() set where the dispatch refuses the descriptor.
 * A one-source descriptor (K1 == K) is planned as called with x2 == NULL: the dispatch reads d->ldx2 whenever x2 is given, so a
 * one-source call that still passes an x2 with ldx2 % 4 != 0 loses its vector loads, which the query cannot see.
 * mi_conv_igemm_bf16w_io_supported asks the same plan, so it too leaves the refusal's text in mi_last_error() when it answers 0. */
#define MI_IGEMM_PLAN_CLASSES 16
typedef struct MiIgemmPlan {
    int kernel;                          /* 0 = igemm_kernel, 1 = igemm_fast_kernel (the register-ring kernel) */
    int bm, bn;                          /* tile */
    int classes;                         /* parity classes of a transposed conv with stride > 1 (stride^2), else 1 */
    int ragged;                          /* output extent not a multiple of the stride: the last class cell is partly dropped */
    int ksplit;                          /* slices of the channel axis; > 1: y is zeroed (unless accumulate) and the slices add atomically */
    int ntap[MI_IGEMM_PLAN_CLASSES];     /* taps that contribute to class c (0 past `classes`) */
    int stages[MI_IGEMM_PLAN_CLASSES];   /* ntap * ceil(K / CK): 32-channel steps (64 for the ring kernel on bf16 activations), all k-slices together */
} MiIgemmPlan;
int mi_conv_igemm_plan(const MiConvDesc* d, int has_wb, int in16, int aligned, MiIgemmPlan* plan);

/* ---- tap-gather GEMM (round 4): the stride-2 Downsample conv (ddpm.py:79), the ConvTranspose2d(4, 2, 1) Upsample (ddpm.py:70) and
 * their data gradients for bf16-stored activations, same contract as mi_conv_igemm (d->transposed = 1: the parity classes of the
 * produced tensor run as blockIdx.z).  x bf16 (K % 64 == 0, one source, ldx % 8 == 0), weights in mi_pack_weights_bf16's fragment order
 * (wfq for the contraction over the master layout's ci, wdq over co), Nc % 64 == 0, power-of-two class grids, N*GH*GW % 64 == 0.
 * Activations by LDS-DMA gathered per tap (the stride is free), private weight streams, one barrier per 128 contraction channels.
 * d->mode = 0: the exact-fp32 instantiation -- x / y fp32 (ldx % 4 == 0), weights from mi_pack_weights_f32frag (wfq32 / wdq32). */
int mi_conv_gt_supported(const MiConvDesc* d);
int mi_conv_gt_tile(const MiConvDesc* d, int* pixels_per_workgroup, int* classes);
int mi_conv_gt(const MiConvDesc* d, const void* x, const void* w_frag, const float* bias, const float* residual,
               void* y, int out_bf16, void* stream);
/* ... and a bf16 copy of the fp32 output from the same epilogue (y_bf16, pixel stride ldy16 elements; bf16 mode, no accumulate) */
int mi_conv_gt_dual(const MiConvDesc* d, const void* x, const void* w_frag, const float* bias, const float* residual,
                    float* y, void* y_bf16, int ldy16, void* stream);

/* ---- 3x3 / stride 1 / pad 1 convolution with an LDS-staged halo tile (bf16 MFMA only) -------
 * Same contract as mi_conv_igemm for the Block conv (ddpm.py:116) and its data gradient
 * (d->transposed = 1 selects the flipped-tap form), but activations are staged once per
 * 9 taps and weights come from a bf16 copy laid out  w[ky][kx][Nc][K]  (k contiguous), made by
 * mi_pack_weights_bf16.  Returns <0 when the descriptor is not supported
 * (check with mi_conv3x3_bf16w_supported and fall back to mi_conv_igemm).
 * Arguments of every entry point of this kernel (refused with <0 otherwise): x, x2 and w 16-byte aligned, ldx % 4 == 0 (ldx2 with
 * x2); ldy % 4 == 0, and ldr % 4 == 0 with a residual; y 16-byte aligned (8-byte when it is written as bf16); residual and bias
 * 16-byte aligned; gsum 8-byte aligned -- the epilogue moves one channel quad per access. */
int mi_conv3x3_bf16w(const MiConvDesc* d, const float* x, const float* x2, const void* w_nk_bf16,
                     const float* bias, const float* residual, float* y, void* stream);
int mi_conv3x3_bf16w_supported(const MiConvDesc* d);
/* 1 when the layer would run the split-K plan (small-M levels; partial sums are combined with fp32 atomics, so
 * the output has to be fp32): the caller keeps such layers' block-internal tensors in fp32. */
int mi_conv3x3_bf16w_uses_splitk(const MiConvDesc* d);
/* profiling attribution: the template arguments of the kernel instantiation a descriptor runs on
 * (conv3x3_halo_kernel<bm, ck, KH, sk, io, waves>, waves = 8 for bm == 256 and for the bm 128 / ck 64 form, else 4) */
int mi_conv3x3_bf16w_tile(const MiConvDesc* d, int io, int* bm, int* ck, int* sk);
/* bf16 activation storage for the ResnetBlock-internal tensors (conv output -> GroupNorm -> conv input and
 * their gradients): io bit 0 = x / x2 are bf16 tensors, bit 1 = y is written as bf16; strides count
 * elements.  3x3 and 1x1; with bit 1 the split-K variant (fp32 atomics) is not used. */
int mi_conv3x3_bf16w_io(const MiConvDesc* d, const void* x, const void* x2, const void* w_nk_bf16,
                        const float* bias, const float* residual, void* y, int io, void* stream);
/* ---- the fused GroupNorm-apply + Mish (+ time bias) + Conv3x3 kernel (BASELINE.json's named kernel) -------------------------
 * ResnetBlock: h = block1(x) = mish(GN(conv(x))); h += mlp(t); h = block2(h) (ddpm.py:112-120,136-143).  Here block2's conv
 * reads the RAW output c1 of block1's conv and applies  mish(c1 * scale[n][c] + shift[n][c]) + tb[n][c]  in registers while it
 * stages its halo tile, so the normalised tensor is never written to or read from HBM.  coef = [3][N][K] (scale = rstd*gamma,
 * shift = beta - mean*scale, tb = the block's time bias) comes from mi_gn_stats_coef, a statistics-only pass over c1 that also
 * writes stats[n][g] = {mean, rstd}.  Forward / sampling path; tiles lie inside one image.  io: 0 = fp32 c1 -> fp32 y, 3 = bf16 ->
 * bf16 (the block-internal storage of bf16 mode). */
/* (mi_gn_stats_coef is declared with the GroupNorm entry points below) */
/* GroupNorm statistics of the NEXT layer from this conv's epilogue (instead of mi_gn_stats_coef's pass over the tensor):
 * mi_conv3x3_bf16w_io_gnsums is mi_conv3x3_bf16w_io that also adds, per sample and 16-channel slab, the sum and the sum of squares of
 * the values it stores (rounded to bf16 when y is bf16) into gsum [N][Nc / 16][2] (zeroed by the caller; Nc % 16 == 0, H*W % 32 == 0).
 * ABI 4: the elements of gsum / sums are 64-bit fixed-point integers with 20 fraction bits (16 bytes per slab; the float* in the
 * signatures is an opaque, 16-byte aligned pointer): they are added with integer atomics, so the totals -- and everything computed
 * from them -- do not depend on the order in which the workgroups arrive;
 * mi_gn_coef_from_sums combines the slabs of each group into stats [N][G][2] = {mean, rstd} (optional) and coef [3][N][C] as
 * mi_gn_stats_coef would have written them (C / G % 16 == 0).  Block -> Block: conv1 + sums, coef, then mi_conv3x3_gn_mish. */
/* mi_conv3x3_bf16w_io that also writes the bf16 copy of its fp32 output (y_bf16, pixel stride ldy16 elements): LinearAttention's
 * to_out conv + residual (ddpm.py:45,152) produces a residual-stream tensor whose bf16 copy the skip connection's consumer, the
 * Downsample conv and the weight gradients read -- one epilogue instead of a conversion pass over y. */
int mi_conv3x3_bf16w_io_dual(const MiConvDesc* d, const void* x, const void* x2, const void* w_nk_bf16, const float* bias,
                             const float* residual, float* y, void* y_bf16, int ldy16, int io, void* stream);
int mi_conv3x3_bf16w_io_gnsums(const MiConvDesc* d, const void* x, const void* x2, const void* w_nk_bf16, const float* bias,
                               const float* residual, void* y, int io, float* gsum, void* stream);
int mi_gn_coef_from_sums(int N, int C, int G, int HW, float eps, const float* sums, const float* gamma, const float* beta,
                         const float* temb, int ldt, float* stats, float* coef, void* stream);
/* ... or skip the coefficient tensor: the fused kernel resolves statistics, affine and time bias (temb [N][ldt], optional) per channel
 * chunk from the sums themselves.  Block -> Block is then two launches: conv1 (+ sums) and this one. */
int mi_conv3x3_gn_mish_sums(const MiConvDesc* d, const void* x, const float* sums, const float* gamma, const float* beta,
                            const float* temb, int ldt, int G, float eps, const void* w_nk_bf16, const float* bias, void* y,
                            int io, void* stream);
int mi_conv3x3_gn_mish_supported(const MiConvDesc* d);
int mi_conv3x3_gn_mish_tile(const MiConvDesc* d, int* bm, int* ck);
int mi_conv3x3_gn_mish(const MiConvDesc* d, const void* x, const float* coef, const void* w_nk_bf16, const float* bias,
                       void* y, int io, void* stream);
/* bf16 shadow copies of every conv weight of the flat fp32 parameter buffer (master layout
 * [tap][Cin][Cout] at float offset `off`): wd = same layout, wf = [tap][Cout][Cin].
 * entries_dev: device array of {int64 off; int32 taps, ci, co, tile0}, tile0 = first tile
 * index of the entry (prefix sum of taps*ceil(ci/T)*ceil(co/T), T = mi_pack_weights_tile()); total_tiles = grid size. */
/* tile edge T the entries' tile0 fields are counted in: an entry owns taps * ceil(ci / T) * ceil(co / T) consecutive tiles */
int mi_pack_weights_tile(void);
/* entries_dev (ABI 2): {int64 off; int32 taps, ci, co, tile0, frag, pad}.  Entries with frag != 0 (ci % 64 == 0 and co % 64 == 0)
 * are also written in MFMA-fragment order for mi_conv3x3_pw (wdq / wfq may both be NULL: no such copies):
 *   wfq[tap][co/32][ci/16][lane][8] = W[tap][ci = 16 kq + 8 (lane >> 5) + e][co = 32 nb + (lane & 31)]   (forward operand)
 *   wdq[tap][ci/32][co/16][lane][8] = W[tap][ci = 32 nb + (lane & 31)][co = 16 kq + 8 (lane >> 5) + e]   (data-gradient operand) */
int mi_pack_weights_bf16(int nent, const void* entries_dev, int total_tiles, const float* master,
                         void* wd_bf16, void* wf_bf16, void* wdq_bf16, void* wfq_bf16, void* stream);
/* ---- 3x3 conv / data gradient for bf16-stored activations with wave-private weight streams (conv_pw.hip; replaces the per-tap
 * workgroup barrier of the kernels above: reference op src/models/ddpm.py:116).  w_frag_bf16 = the layer's slice of wfq (forward) or
 * wdq (d->transposed = 1: data gradient, flipped taps).  Needs W in {8, 16, 32} with 128-pixel row tiles (N*H*W % 128 == 0),
 * K % 64 == 0, K1 % 64 == 0, Nc % 64 == 0, ldy % 8 == 0 (pw_ok / pw_launch in conv_pw.hip are the authority). */
int mi_conv3x3_pw_supported(const MiConvDesc* d);
/* ... for fp32 x / x2 (the residual stream as it is; pixel strides in floats, % 4 == 0): rounded to bf16 once while staged; gsum
 * (optional): the GroupNorm sums of mi_conv3x3_pw_gnsums */
int mi_conv3x3_pw_x32_supported(const MiConvDesc* d);
int mi_conv3x3_pw_x32_tile(const MiConvDesc* d);
int mi_conv3x3_pw_x32(const MiConvDesc* d, const float* x, const float* x2, const void* w_frag_bf16, const float* bias,
                      const float* residual, void* y, int out_bf16, float* gsum, void* stream);
/* ... and in exact-fp32 mode (d->mode = 0; Unet.compute_mode = "fp32", the reference's default precision): the same kernel on
 * v_mfma_f32_32x32x2_f32 with fp32 x / x2 / y and fp32 weights in fragment order, written by mi_pack_weights_f32frag from the table
 * of mi_pack_weights_bf16:  wfq32[tap][co/32][ci/8][lane][4] = W[tap][ci = 8 ko + 4 (lane >> 5) + j][co = 32 nb + (lane & 31)],
 * wdq32[tap][ci/32][co/8][lane][4] = W[tap][ci = 32 nb + (lane & 31)][co = 8 ko + 4 (lane >> 5) + j].  K % 32 == 0, K1 % 32 == 0. */
int mi_conv3x3_pw_f32_tile(const MiConvDesc* d);
int mi_conv3x3_pw_f32(const MiConvDesc* d, const float* x, const float* x2, const float* w_frag_f32, const float* bias,
                      const float* residual, float* y, void* stream);
int mi_conv1x1_pw_x32_supported(const MiConvDesc* d);     /* ... reading fp32 x / x2 (strides in floats, % 4): the fp32 stream gradient, inference */
int mi_conv1x1_pw_x32(const MiConvDesc* d, const float* x, const float* x2, const void* w_frag_bf16, const float* bias,
                      const float* residual, void* y, int out_bf16, void* stream);
/* split-K launches of the 3x3 tile kernel (mi_conv3x3_pw*; the layers whose tiles would leave CUs without a workgroup: the sampler at B = 64,
   BASELINE configs[2] at 32 images per GPU): ws = device memory the caller zeroed once and keeps alive (64 KB of flags + the fp32 partial tiles;
   a launch that does not fit runs unsplit), registered for the calling thread's device; launches that use it must be ordered on one stream.
   null / 0: no split launches.  mi_conv3x3_pw_splitk: the split a launch would use now (1: none) + 16 x its pixel tile. */
int mi_conv_pw_set_splitk_workspace(void* ws, size_t bytes);
int mi_conv3x3_pw_splitk(const MiConvDesc* d, int var, int in32);
int mi_debug_conv_pw_splitk(int mode);                     /* tests: 0 off, 1 the rule, 2 / 4 that split wherever the geometry allows; -> previous */
/* inference: channel LayerNorm (reference src/models/ddpm.py:85-95) + the bias-free 1x1 conv behind it (to_qkv, :151) in one launch -- the
   normalised tensor is never written.  x fp32 [M][ldx], ln_g / ln_b [K], K = 128 / 256 / 512, y bf16 [M][ldy] */
int mi_ln_conv1x1_pw_supported(const MiConvDesc* d);
int mi_ln_conv1x1_pw(const MiConvDesc* d, const float* x, const float* ln_g, const float* ln_b, float eps, const void* w_frag_bf16,
                     const float* bias, void* y_bf16, void* stream);
/* ... that also writes the normalised tensor (bf16 [M][ldl]): training -- to_qkv's weight gradient reads it, no LayerNorm launch */
int mi_ln_conv1x1_pw_dual(const MiConvDesc* d, const float* x, const float* ln_g, const float* ln_b, float eps, const void* w_frag_bf16,
                          const float* bias, void* y_bf16, void* ln_bf16, int ldl, void* stream);
int mi_conv1x1_pw_f32_supported(const MiConvDesc* d);     /* the 1x1 convs in exact-fp32 mode: K % 64 == 0, K1 % 64 == 0, Nc % 64 == 0 */
int mi_conv1x1_pw_f32(const MiConvDesc* d, const float* x, const float* x2, const float* w_frag_f32, const float* bias,
                      const float* residual, float* y, void* stream);
int mi_pack_weights_f32frag(int nent, const void* entries_dev, int total_tiles, const float* master, float* wdq32, float* wfq32,
                            void* stream);
int mi_debug_conv_pw_tile(int pt);               /* tests: force the pixel tile (64 / 128 / 256), 0 = automatic */
int mi_debug_conv_pw_auto256(int min_workgroups); /* A/B switch: the automatic pick takes 256-pixel tiles from this many workgroups up (0 = never; default 256) */
int mi_debug_conv1x1_pw_nloop(int on);          /* A/B switch: 0 = the bf16 -> bf16 K = 128 1x1 conv (to_qkv) always on the 2-D grid, 1 = the channel-tile loop from 1024 pixel tiles up (default), 2 = from any grid (tests), < 0 = query only; returns the previous value */
int mi_conv3x3_pw_tile(const MiConvDesc* d);      /* pixels per workgroup the launch would use: 256 (grids that still fill the chip), 128, or 64 for small grids; 0 = unsupported */
int mi_conv3x3_pw(const MiConvDesc* d, const void* x, const void* x2, const void* w_frag_bf16, const float* bias,
                  const float* residual, void* y, int out_bf16, void* stream);
/* ... whose epilogue also adds the sum and the sum of squares of the values it stores (rounded to bf16 when y is bf16), per sample and
 * 16-channel slab, into gsum [N][Nc/16][2] (zeroed by the caller, Nc % 16 == 0): the statistics of the GroupNorm that follows
 * (mi_gn_coef_from_sums) without a pass over y -- one atomic pair per slab, image and workgroup. */
int mi_conv3x3_pw_gnsums(const MiConvDesc* d, const void* x, const void* x2, const void* w_frag_bf16, const float* bias,
                         const float* residual, void* y, int out_bf16, float* gsum, void* stream);
/* BASELINE.json's named kernel on this structure (reference src/models/ddpm.py:112-120,136-143):
 *   y = conv3x3(mish(x * scale[n][c] + shift[n][c]) + tb[n][c]) + bias,
 * x = the RAW bf16 output of block1's conv, coef [3][N][K] fp32 = scale, shift, tb (mi_gn_coef_from_sums or mi_gn_stats_coef).  The
 * transform is applied ONCE per staged element: a wave rewrites, in place in LDS, the activation pieces it requested itself (after its
 * own counted wait, before the chunk barrier publishes them); rows outside the image stay zero.  Tiles lie inside one image
 * (W in {16, 32}); the normalised tensor never exists in HBM. */
int mi_conv3x3_pw_gn_mish_supported(const MiConvDesc* d);
int mi_conv3x3_pw_gn_mish_tile(const MiConvDesc* d);          /* pixels per workgroup the fused variants would use (128 / 64; 0: not supported) */
int mi_conv3x3_pw_gn_mish(const MiConvDesc* d, const void* x, const float* coef, const void* w_frag_bf16, const float* bias,
                          void* y, int out_bf16, void* stream);
/* ... or without the coefficient tensor: scale / shift are resolved per channel chunk inside the kernel from the sums the producing
 * conv's epilogue left (sums [N][K/16][2], mi_conv3x3_pw_gnsums / mi_conv3x3_bf16w_io_gnsums), gamma, beta and the time-bias rows
 * temb [N][ldt] (optional) with mi_gn_coef_from_sums' arithmetic.  K / G in {16, 32, 64}.  Block -> Block = two launches. */
int mi_conv3x3_pw_gn_mish_sums(const MiConvDesc* d, const void* x, const float* sums, const float* gamma, const float* beta,
                               const float* temb, int ldt, int G, float eps, const void* w_frag_bf16, const float* bias,
                               void* y, int out_bf16, void* stream);
/* The same two for fp32-STORED activations (block storage fp32; x = the raw fp32 output of the previous conv, pixel stride in floats,
 * % 4 == 0): the transform is applied to the fp32 values while they pass through registers on their way to the bf16 tile (one rounding,
 * no LDS read-modify-write).  y fp32 or bf16.  The canonical shape of BASELINE.json's named kernel in the regime SURVEY 8(d)(ii) calls balanced. */
int mi_conv3x3_pw_x32_gn_mish_supported(const MiConvDesc* d);
int mi_conv3x3_pw_x32_gn_mish_tile(const MiConvDesc* d);      /* pixels per workgroup (128 / 64; 0: not supported) */
int mi_conv3x3_pw_x32_gn_mish(const MiConvDesc* d, const float* x, const float* coef, const void* w_frag_bf16, const float* bias,
                              void* y, int out_bf16, void* stream);
int mi_conv3x3_pw_x32_gn_mish_sums(const MiConvDesc* d, const float* x, const float* sums, const float* gamma, const float* beta,
                                   const float* temb, int ldt, int G, float eps, const void* w_frag_bf16, const float* bias,
                                   void* y, int out_bf16, void* stream);
/* ---- 1x1 convs with K % 128 == 0 input channels on the same machinery (to_qkv, to_out + residual, res_conv -- also over the skip
 * concat's two sources, x2 = channels K1 .. K - 1 with K1 % 128 == 0 -- and their data gradients; reference src/models/ddpm.py:134,151-152):
 * 128 (or 64) pixels x 128 output channels per workgroup, the activation tile double-buffered per 128-channel chunk by LDS-DMA, weight
 * fragments straight into registers per wave, whole rows leave through LDS.  w_frag_bf16 = the layer's slice of wfq (forward) / wdq
 * (data gradient); y fp32 or bf16 (out_bf16); y_bf16 (optional, fp32 y, no accumulate): the bf16 copy of y from the same epilogue
 * (pixel stride ldy16). */
int mi_conv1x1_pw_supported(const MiConvDesc* d);
int mi_conv1x1_pw(const MiConvDesc* d, const void* x, const void* x2, const void* w_frag_bf16, const float* bias, const float* residual,
                  void* y, int out_bf16, void* y_bf16, int ldy16, void* stream);

/* ---- the 3-channel ends of the UNet (fp32 VALU, bound by the wide tensor they stream) ------------
 * Conv2d(Cin<=4, Cout, ks, padding=ks/2), ks = 3 (downs.0.0.block1, ddpm.py:116,208) or 1 (its res_conv,
 * ddpm.py:134): forward and weight gradient; w / dW in the tap-major layout [ks][ks][Cin][Cout].
 * Forward: Cout % 4 == 0 and Cout/4 divides 256.  Weight gradient: Cout in {64, 128, 256} whose reduce area of
 * 3 * ks*ks*Cin * (Cout/4) float4 fits 48 KiB (ks = 1: all; ks = 3: Cin * Cout <= 455, so Cin = 1 admits 256, Cin = 4 only 64);
 * with a workspace of mi_conv_small_wgrad_workspace(ks*ks*Cin*Cout) bytes the per-workgroup partial tiles are
 * summed in a fixed order (deterministic), without one they are added with fp32 atomics. */
int mi_conv_small_cin_fwd(int ks, int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* w,
                          const float* bias, float* y, int ldy, void* stream);
int mi_conv_small_cin_wgrad(int ks, int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* dy,
                            int lddy, float* dW, void* workspace, size_t ws_bytes, void* stream);
size_t mi_conv_small_wgrad_workspace(int outputs);
/* Round 4: the wide (Cout-channel) tensor stored as bf16, like every other block-internal tensor of bf16 mode (the reference keeps
 * c1 = conv(x) and its gradient in fp32, ddpm.py:116-120; x, w, dW stay fp32, the arithmetic is the same fp32 FMA chain, the output
 * is rounded once / dy is widened on load).  y_bf16 / dy_bf16 = 1 needs the whole-row-tile kernels: ks = 3, W a power of two <= 64,
 * H*W a power of two, ldx == 4, 16-byte aligned x, Cout in {64, 128, 256} under the weight gradient's 48 KiB rule above (Cin = 1: 256 too; a forward alone
 * takes any Cout <= 256) -- mi_conv_small_cin_bf16_supported answers for both. */
int mi_conv_small_cin_bf16_supported(int ks, int N, int H, int W, int Cin, int Cout, int ldx);
/* round 6, inference -- LinearAttention (reference ddpm.py:146-165) folded into its to_out conv: out = ctx^T q is linear in q, so to_out(out) is a 1x1
   conv of q with per-sample weights W_eff[b] = W_out blockdiag(ctx_h^T).  mi_linattn_fold_fwd: qkv bf16 [B][n][3 * heads * 32], w_out_bf16 = to_out's
   bf16 weight rows [C][heads * 32] (mi_pack_weights_bf16's wf) -> weff bf16 [B][C * heads * 32] in fragment order; mi_conv1x1_pw_batched: mi_conv1x1_pw with the weights of sample b at
   w_frag_bf16 + b * wbatch elements (x = qkv, d->ldx = 3 * hidden, d->K = hidden: the q channels) */
int mi_linattn_fold_fwd(int B, int n, int heads, const void* qkv_bf16, const void* w_out_bf16, int C, void* weff_bf16, void* stream);
int mi_conv1x1_pw_batched(const MiConvDesc* d, const void* x, const void* w_frag_bf16, int wbatch, const float* bias, const float* residual,
                          void* y, int out_bf16, void* y_bf16, int ldy16, void* stream);
/* round 6: backward of the C -> 3 conv (final_conv.1, reference ddpm.py:235) in one pass over (x, dy): weight gradient and data gradient */
int mi_conv1x1_small_cout_bwd(int M, int C, int Cs, const void* x, int ldx, int x_bf16, const float* dy, int lddy, const float* w,
                              float* dW, void* dx, int lddx, int dx_bf16, int accumulate_dx, void* workspace, size_t ws_bytes, void* stream);
/* round 6, inference: final_conv (reference ddpm.py:232-235) -- the Block's GroupNorm-apply + Mish inside the Conv2d(dim, channels, 1)'s load: x = the
   Block conv's bf16 output, sums = what its epilogue left (mi_conv3x3_pw_gnsums); C = 64 / 128, (C / G) % 16 == 0 */
int mi_conv1x1_small_cout_gn_supported(int C, int Cs, int G);
int mi_conv1x1_small_cout_gn_fwd(int M, int HW, int C, int Cs, const void* x_bf16, int ldx, const void* sums, const float* gamma,
                                 const float* beta, int G, float eps, const float* w, const float* bias, float* y, int ldy, void* stream);
/* round 6: the first ResnetBlock's 3x3 conv and its res_conv (Conv2d(Cin, Cout, 1), reference ddpm.py:134,143) on the same image in one launch */
int mi_conv_small_cin_fwd_dual_supported(int N, int H, int W, int Cin, int Cout, int ldx);
int mi_conv_small_cin_fwd_dual(int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* w3, const float* bias3,
                               void* y3, int ldy3, int y3_bf16, const float* w1, const float* bias1, float* y1, int ldy1, void* stream);
/* ... that also does a forward's two chores whose consumers are later launches (this is a forward's first launch): zero-fills the pool of GroupNorm
   sums, gathers the denoise step's time-bias rows gather_dst[b][:] = gather_src[gather_idx[b]][:] (int64 indices); either may be null */
int mi_conv_small_cin_fwd_dual_chores(int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* w3, const float* bias3,
                                    void* y3, int ldy3, int y3_bf16, const float* w1, const float* bias1, float* y1, int ldy1,
                                    void* zero, size_t zero_bytes, const float* gather_src, const void* gather_idx, float* gather_dst,
                                    int gather_row, int gather_n, void* stream);
int mi_conv_small_cin_fwd_io(int ks, int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* w,
                             const float* bias, void* y, int ldy, int y_bf16, void* stream);
int mi_conv_small_cin_wgrad_io(int ks, int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const void* dy,
                               int lddy, int dy_bf16, float* dW, void* workspace, size_t ws_bytes, void* stream);
/* the 3x3 forms without workspace */
int mi_conv3x3_small_cin_fwd(int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* w,
                             const float* bias, float* y, int ldy, void* stream);
int mi_conv3x3_small_cin_wgrad(int N, int H, int W, int Cin, int Cout, const float* x, int ldx, const float* dy,
                               int lddy, float* dW, void* stream);
/* Conv2d(C, Cs<=4, 1) (final_conv.1, ddpm.py:236), weights w[C][Cs], C in {32, 64, 128, 256}.  op 0: y = x w + bias
 * (C <= 128); op 1: dx (+)= dy w^T; op 2: dW += x^T dy (a = x, b = dy; C >= 64; workspace of
 * mi_conv_small_wgrad_workspace(4*C) bytes as above). */
int mi_conv1x1_small_cout(int op, int M, int C, int Cs, const float* a, int lda, const float* b, int ldb,
                          const float* w, const float* bias, float* out, int ldo, int accumulate, void* stream);
int mi_conv1x1_small_cout_ws(int op, int M, int C, int Cs, const float* a, int lda, const float* b, int ldb,
                             const float* w, const float* bias, float* out, int ldo, int accumulate,
                             void* workspace, size_t ws_bytes, void* stream);
/* wide_bf16 = 1 (round 4): the C-channel tensor (x of op 0 / 2, dx of op 1: final_conv.0's output and its gradient) is bf16; the
 * Cs-channel side, the weights and the arithmetic stay fp32 */
int mi_conv1x1_small_cout_io(int op, int M, int C, int Cs, const void* a, int lda, const float* b, int ldb,
                             const float* w, const float* bias, void* out, int ldo, int accumulate, int wide_bf16,
                             void* workspace, size_t ws_bytes, void* stream);

/* ---- weight gradient (aten::convolution_backward, weight part) -----------------------
 *   dW[ky][kx][i][j] += sum_{n,y,x} P[n,py,px,i] * Q[n,qy,qx,j]
 * (y,x) runs over the DH x DW grid of the non-gathered operand; the gathered operand is
 * read at (y*stride - pad + ky, x*stride - pad + kx) of its GH x GW grid.
 * gather_i=1: P gathered (Conv2d: P = layer input, Q = grad of output);
 * gather_i=0: Q gathered (ConvTranspose2d: P = layer input, Q = grad of output).
 * P channel i comes from P when i < I1 else from P2 at i-I1.  dW is accumulated with
 * fp32 atomics (split over the pixel axis), so zero it first.
 */
typedef struct MiWgradDesc {
    int N;
    int GH, GW;          /* gathered operand grid */
    int DH, DW;          /* direct operand grid (loop grid) */
    int Ci, Cj;
    int KH, KW, stride, pad;
    int gather_i;
    int mode;
    int I1;
    int ldp, ldp2, ldq;
} MiWgradDesc;

int mi_conv_wgrad(const MiWgradDesc* d, const float* P, const float* P2, const float* Q,
                  float* dW, void* stream);
/* What mi_conv_wgrad (slab = 0) / mi_conv_wgrad_slabs (slab = 1) decide for d (read-only; the launch comes from the same function).
 * aligned: P, P2 and Q are 16-byte aligned (the pitches are read from d).  Non-zero with mi_last_error() set where d is refused
 * (non-positive sizes among the reasons: mi_conv_wgrad refuses them too).  As for the convolution, I1 == Ci is planned as called
 * with P2 == NULL; the launch reads d->ldp2 whenever P2 is given. */
typedef struct MiWgradPlan {
    int fast;            /* 1 = wgrad_fast_kernel (the register-ring kernel), 0 = wgrad_kernel */
    int big;             /* 128 x 128 channel tiles (Ci >= 128 and Cj >= 128), else 64 x 64 */
    int splits, chunk;   /* slices of the pixel axis and pixels per slice (a multiple of 32) */
    int xcd_map;         /* ring kernel: 1-D grid that keeps a slice's workgroups on one XCD (splits >= 8) */
    int grid;            /* workgroups of the launch (with xcd_map: splits rounded up to 8, the surplus returns at once) */
} MiWgradPlan;
int mi_conv_wgrad_plan(const MiWgradDesc* d, int aligned, int slab, MiWgradPlan* plan);

/* 3x3 / stride 1 / pad 1 Conv2d weight gradient on bf16 MFMA with image-major contraction vectors
 * (needs N % 8 == 0, channel counts % 32 == 0; query first, else use mi_conv_wgrad). */
int mi_conv3x3_wgrad(const MiWgradDesc* d, const float* P, const float* P2, const float* Q, float* dW, void* stream);
int mi_conv3x3_wgrad_supported(const MiWgradDesc* d);
/* profiling attribution: wgrad3x3_kernel<nj, KH, io> and the number of k-slices (= partial tiles per output tile) */
int mi_conv3x3_wgrad_tile(const MiWgradDesc* d, int* nj, int* splits);
/* measurement aid for per-kernel event timing: 0 = normal, 1 = launch only the contraction kernel, 2 = only the partial-tile
 * reduce (one call with 1 followed by one with 2 == one normal call).  Process-global; reset to 0 after use. */
int mi_debug_wgrad3x3_phase(int phase);
/* Same, but the k-slices write partial tiles to a caller-provided scratch buffer that a second
 * (deterministic) kernel sums into dW -- 2.4x cheaper than fp32 atomics here.  Size from
 * mi_conv3x3_wgrad_workspace(); a null / too small workspace falls back to atomics. */
size_t mi_conv3x3_wgrad_workspace(const MiWgradDesc* d);
int mi_conv3x3_wgrad_ws(const MiWgradDesc* d, const float* P, const float* P2, const float* Q, float* dW,
                        void* workspace, size_t ws_bytes, void* stream);
/* ... and additionally dbias[j] += sum over pixels of Q[., j] (the conv's bias gradient) from the
 * same pass over Q (replaces a separate mi_colsum over the gradient tensor). */
int mi_conv3x3_wgrad_bias(const MiWgradDesc* d, const float* P, const float* P2, const float* Q, float* dW,
                          float* dbias, void* workspace, size_t ws_bytes, void* stream);
/* ... with bf16-stored operands: io bit 0 = P / P2 bf16, bit 1 = Q bf16 (3x3 only) */
int mi_conv3x3_wgrad_io(const MiWgradDesc* d, const void* P, const void* P2, const void* Q, float* dW,
                        float* dbias, void* workspace, size_t ws_bytes, int io, void* stream);

/* 3x3 / stride 1 / pad 1 Conv2d weight gradient (ddpm.py:116) for bf16-STORED operands (P / P2 / Q are bf16 tensors, strides in
 * elements, % 8 == 0): rows go L2 -> LDS by LDS-DMA, MFMA operands come out of LDS through the transposing ds_read_b64_tr_b16, one
 * workgroup accumulates all nine taps of a 64 x 128 (ci x co) tile over its slice of the pixel axis; slices are summed in a fixed
 * order by a second kernel through `workspace` (mi_conv3x3_wgrad_tr_workspace bytes).  dW += result, layout [3][3][Ci][Cj].
 * Needs W in {8,16,32,64}, H % (64/W) == 0, N*H*W % 64 == 0, Ci % 64 == 0, I1 % 64 == 0, Cj % 32 == 0 (query _supported).
 * d->mode = 0 (exact-fp32 mode): P / P2 / Q are fp32 tensors (strides % 4 == 0) and the contraction runs on v_mfma_f32_32x32x2_f32 with
 * plain ds_read_b32 fragments of pixel-major fp32 tiles -- same tiles, k-slices, reduce and batching (one mode per batch). */
int mi_conv3x3_wgrad_tr_supported(const MiWgradDesc* d);
size_t mi_conv3x3_wgrad_tr_workspace(const MiWgradDesc* d);
int mi_conv3x3_wgrad_tr_splits(const MiWgradDesc* d);
int mi_conv3x3_wgrad_tr(const MiWgradDesc* d, const void* P, const void* P2, const void* Q, float* dW,
                        void* workspace, size_t ws_bytes, void* stream);
/* Up to 8 independent layers in ONE launch, each on a share of the workgroups proportional to its MFMA work.  The partial-tile
 * volume of a layer is (its workgroups) x 288 KB, so eight layers side by side write an eighth of what eight full-chip launches
 * write, and layers with at least as many tiles as workgroups accumulate straight into dW (no k-slices, no reduce).  descs: array
 * of n descriptors; P / P2 / Q / dW: arrays of n device pointers (P2 entries may be null); the layers' weight gradients must not
 * alias each other.  Backward defers the Block convs' weight gradients and flushes them through this entry point. */
size_t mi_conv3x3_wgrad_tr_batch_workspace(int n, const MiWgradDesc* descs);
int mi_conv3x3_wgrad_tr_batch(int n, const MiWgradDesc* descs, const void* const* P, const void* const* P2,
                              const void* const* Q, float* const* dW, void* workspace, size_t ws_bytes, void* stream);
/* The 1x1 convolutions' weight gradients (to_qkv / to_out / res_conv, ddpm.py:134,151-152) the same way: dW[Ci][Cj] += X^T dY over
 * all pixels, up to 8 layers per launch on shares of the workgroups proportional to the bytes they stream (these are HBM-bound).
 * P / P2 are bf16 tensors; Q is bf16 (q_is_fp32[i] = 0) or the fp32 residual-stream gradient (1: rows are DMA'd raw and converted
 * in LDS, and dbias[i] (optional) += column sums of Q -- the conv's bias gradient, replacing a separate mi_colsum pass).
 * Needs N*H*W % 64 == 0, Ci % 64 == 0, I1 % 64 == 0, Cj % 32 == 0, ldp % 8 == 0, ldq % 8 (bf16) / % 4 (fp32) == 0.
 * mode 0 (round 4; Unet.compute_mode = "fp32"): P / P2 and Q are fp32 tensors (q_is_fp32 = 1, ldp / ldp2 / ldq % 4 == 0), the products run
 * on v_mfma_f32_32x32x2_f32 -- an fp32 fmaf chain per k-slice, slices added in a fixed order; one mode per batch. */
int mi_conv1x1_wgrad_tr_supported(const MiWgradDesc* d, int q_is_fp32);
size_t mi_conv1x1_wgrad_tr_batch_workspace(int n, const MiWgradDesc* descs, const int* q_is_fp32);
int mi_conv1x1_wgrad_tr_batch(int n, const MiWgradDesc* descs, const int* q_is_fp32, const void* const* P,
                              const void* const* P2, const void* const* Q, float* const* dW, float* const* dbias,
                              void* workspace, size_t ws_bytes, void* stream);
int mi_debug_wgrad1x1_tr_phase(int phase);
int mi_debug_wgrad1x1_tr_blocks(int blocks);
/* measurement aid, as mi_debug_wgrad3x3_phase: 1 = contraction kernel only, 2 = reduce only, 0 = both */
int mi_debug_wgrad_tr_phase(int phase);
/* test aid: plan the k-slices for `blocks` workgroups instead of one per CU (0 = default) */
int mi_debug_wgrad_tr_blocks(int blocks);

/* The stride-2 layers' weight gradients for bf16-stored operands on the same machinery (csrc/wgrad_s2_tr.hip):
 *   Downsample Conv2d(C, C, 3, 2, 1), ddpm.py:70:           descriptor KH = KW = 3, stride 2, pad 1, gather_i = 1, (GH, GW) = X's grid =
 *                                                            2 x (DH, DW) = dY's grid, P = X, Q = dY;
 *   Upsample ConvTranspose2d(C, C, 4, 2, 1), ddpm.py:79:     KH = KW = 4, stride 2, pad 1, gather_i = 0, (GH, GW) = dY's grid =
 *                                                            2 x (DH, DW) = X's grid, P = X, Q = dY.
 * dW[KH][KW][Ci][Cj] += result.  The 2x-resolution tensor is staged as even / odd column planes (LDS-DMA places every 16-byte piece
 * individually), so the stride costs nothing; up to 8 layers per launch.  Needs DW in {8,16,32}, DH % (64/DW) == 0,
 * N*DH*DW % 64 == 0, channels of the 2x tensor % 64 == 0, of the other % 32 == 0, strides % 8 == 0 (query _supported). */
int mi_conv_s2_wgrad_tr_supported(const MiWgradDesc* d);
size_t mi_conv_s2_wgrad_tr_batch_workspace(int n, const MiWgradDesc* descs);
int mi_conv_s2_wgrad_tr_batch(int n, const MiWgradDesc* descs, const void* const* P, const void* const* Q, float* const* dW,
                              void* workspace, size_t ws_bytes, void* stream);
int mi_debug_wgrad_s2_tr_phase(int phase);

/* The three batched entry points above with a trailing `flags` (flags = 0 is exactly the call above: dW += result).
 *   MI_WGRAD_STORE   dW = result.  Every element of a layer's dW has one writer per call (the reduce kernel, or the contraction's
 *                    epilogue when the layer has a single k-slice), so a gradient buffer that is rewritten every step needs neither
 *                    a zero fill nor the read of those zeros.  Nothing outside [KH][KW][Ci][Cj] is written; the sums and their order
 *                    are those of the accumulating call.  dbias (1x1) is still an atomic add. */
#define MI_WGRAD_STORE 1u
int mi_conv3x3_wgrad_tr_batch_ex(int n, const MiWgradDesc* descs, const void* const* P, const void* const* P2,
                                 const void* const* Q, float* const* dW, void* workspace, size_t ws_bytes, void* stream, unsigned flags);
int mi_conv1x1_wgrad_tr_batch_ex(int n, const MiWgradDesc* descs, const int* q_is_fp32, const void* const* P,
                                 const void* const* P2, const void* const* Q, float* const* dW, float* const* dbias,
                                 void* workspace, size_t ws_bytes, void* stream, unsigned flags);
int mi_conv_s2_wgrad_tr_batch_ex(int n, const MiWgradDesc* descs, const void* const* P, const void* const* Q, float* const* dW,
                                 void* workspace, size_t ws_bytes, void* stream, unsigned flags);

/* Exact-fp32 mode (d->mode = 0), round 6: the same two layers' weight gradients (Conv2d(C, C, 3, 2, 1) of Downsample, ConvTranspose2d(C, C, 4,
 * 2, 1) of Upsample; reference src/models/ddpm.py:70,79 -- aten::convolution_backward (weight)) as k x k gathered problems of the exact-fp32
 * 1x1 weight-gradient kernel (v_mfma_f32_32x32x2_f32 = an fp32 fmaf chain), up to eight taps per launch.  P fp32 [N][..][Ci], Q fp32
 * [N][..][Cj], d->gather_i: P lies on the big grid (GH = 2 DH), else Q; dW [KH][KW][Ci][Cj] += ...; workspace from _workspace(). */
int mi_conv_s2_wgrad_f32_supported(const MiWgradDesc* d);
size_t mi_conv_s2_wgrad_f32_workspace(const MiWgradDesc* d);
int mi_conv_s2_wgrad_f32(const MiWgradDesc* d, const float* P, const float* Q, float* dW, void* workspace, size_t ws_bytes, void* stream);
/* measurement aid (tools/cu_hog.py): `blocks` workgroups of 256 threads that stay resident on `stream` for `usec` microseconds -- mode 0
 * an ALU spin, 1 a streaming copy over buf (2 x per_wg_floats floats per workgroup), 2 the same copy with a gradient all-reduce's duty
 * cycle (0.5 ms of every 5 ms) -- to see how a training step behaves while another stream's kernel shares the chip */
int mi_debug_spin(int blocks, int usec, float* buf, size_t per_wg_floats, int mode, void* stream);
/* measurement aid (bench.py's config.sclk_mhz_under_mfma): `blocks` workgroups issue back-to-back bf16 MFMAs for `usec` microseconds;
 * out3 (device, 3 x uint64): shader-clock ticks (s_memtime) and 100 MHz wall-clock ticks workgroup 0 saw across its loop, and a sink word */
int mi_debug_clock_probe(int blocks, int usec, unsigned long long* out3, void* stream);

/* One pass over an fp32 [M][C] tensor: y_bf16 (optional) = bf16(x), colsum (optional)[c] += sum_m x[m][c].  Backward: a residual-
 * stream gradient that the LDS-DMA weight-gradient kernels want bf16-stored and whose column sums are the conv's bias gradient.
 * workspace (optional; mi_f32_to_bf16_colsum_workspace bytes, 16-byte aligned) holds per-workgroup partial sums so that the pass runs
 * on a full grid and a second small pass adds them; without it the sums are added atomically from at most 64 workgroups. */
size_t mi_f32_to_bf16_colsum_workspace(size_t M, int C);
int mi_f32_to_bf16_colsum(size_t M, int C, const float* x, int ldx, void* y_bf16, int ldy, float* colsum, void* workspace,
                          size_t ws_bytes, void* stream);
/* ... the first pass only: one row of column sums per workgroup into part[*rows][C] (every row written; mi_f32_to_bf16_colsum_workspace
 * bytes), to be added by mi_rowsum_batch together with the other deferred reductions of a backward pass.  *rows = 0: the tensor is too
 * small for partial rows (M < 4096), nothing was done. */
int mi_f32_to_bf16_colsum_part(size_t M, int C, const float* x, int ldx, void* y_bf16, int ldy, float* part, size_t part_bytes,
                               int* rows, void* stream);
/* out[c] += sum_m x[m*ld + c]  (bias gradients) */
int mi_colsum(int M, int C, const float* x, int ld, float* out, void* stream);
/* The same sums with no atomics: every row block stores a partial row into ws (mi_colsum_ordered_workspace(M, C) bytes, any content),
 * a second launch adds them in order.  Two runs give the same bits. */
size_t mi_colsum_ordered_workspace(int M, int C);
int mi_colsum_ordered(int M, int C, const float* x, int ld, float* out, void* ws, size_t ws_bytes, void* stream);
/* mi_conv_wgrad's generic kernel with no atomics: each slice of the pixel axis STORES its tiles into its own slab of ws
 * ([slices][KH*KW][Ci][Cj] floats, mi_conv_wgrad_slabs_workspace(d) bytes, any content) and a second launch adds the slabs onto dW in
 * slice order.  Same descriptors, same slicing; two runs give the same bits. */
size_t mi_conv_wgrad_slabs_workspace(const MiWgradDesc* d);
int mi_conv_wgrad_slabs(const MiWgradDesc* d, const float* P, const float* P2, const float* Q, float* dW, void* ws, size_t ws_bytes,
                        void* stream);
/* dst[c] += sum_{r < rows} src[r*ld + c], c < cols, for up to MI_ROWSUM_MAX items in ONE launch: the second pass of the reductions
 * that leave one partial row per workgroup (mi_chan_layernorm_bwd_part) -- device-scope atomics on one address serialise, so 512
 * workgroups adding to the same C addresses cost ~10 us at the end of every launch; here an address receives rows / 64 atomics. */
#define MI_ROWSUM_MAX 16
typedef struct { const float* src; float* dst; int rows, cols, ld, pad_; } MiRowSum;
int mi_rowsum_batch(int n, const MiRowSum* items, void* stream);
/* base[off .. off + cnt) = 0 for the n (off, cnt) pairs (int64, in floats; cnt may be 0) of a table in DEVICE memory, in one kernel
 * launch (a kernel node under graph capture, never a memset node).  The flat gradient buffer's zero fill without the weight gradients
 * that MI_WGRAD_STORE writes outright.  The ranges are the caller's: nothing checks them against the buffer. */
int mi_zero_ranges(const long long* table_dev, int n, float* base, void* stream);

/* ---- GroupNorm(8)+Mish (+time bias, +residual) ---------------------------------------
 * Block's GroupNorm->Mish (ddpm.py:116,62-64), the time-embedding add `h += mlp(t)`
 * (ddpm.py:139-140) and ResnetBlock's `h + res_conv(x)` (ddpm.py:143) in one pass:
 *   y = mish( (x-mean_{n,g}) * rstd_{n,g} * gamma[c] + beta[c] ) + temb[n,c] + residual
 * stats[n][g] = {mean, rstd} is written for backward.  HW*C/G elements per (n,g).
 */
typedef struct MiGnDesc {
    int N, HW, C, G;
    float eps;
    int ldx, ldy, ldr;
} MiGnDesc;

int mi_gn_mish_fwd(const MiGnDesc* d, const float* x, const float* gamma, const float* beta,
                   const float* temb, int ldt, const float* residual, float* y, float* stats,
                   void* stream);
/* dx = grad wrt x.  dgamma/dbeta/dbias (each [C]) are accumulated atomically; dtemb[n*ldt+c]
 * is stored (= sum_hw dout) when non-null; dbias (sum_{n,hw} dx, the producing conv's bias
 * gradient) when non-null.  The residual branch's gradient is dout itself. */
int mi_gn_mish_bwd(const MiGnDesc* d, const float* x, const float* stats, const float* gamma,
                   const float* beta, const float* dout, int lddo, float* dx, int lddx,
                   float* dgamma, float* dbeta, float* dtemb, int ldt, float* dbias,
                   void* stream);

/* bf16 storage variants.  fwd io: bit 0 = x bf16, bit 1 = y bf16.  bwd io: bit 0 = x bf16, bit 1 = dx bf16,
 * bit 2 = dout bf16.  gamma/beta/temb/residual/stats and all parameter gradients stay fp32. */
int mi_gn_mish_fwd_io(const MiGnDesc* d, const void* x, const float* gamma, const float* beta, const float* temb,
                      int ldt, const float* residual, void* y, float* stats, int io, void* stream);
/* mi_gn_mish_fwd_io that also writes y rounded to bf16 into y16 (pixel stride ldy16 elements): the residual stream stays fp32 in y,
 * the next layer's bf16-MFMA kernels read the copy (ddpm.py:116,143: the ResnetBlock output feeds the next block's convs). */
int mi_gn_mish_fwd_dual(const MiGnDesc* d, const void* x, const float* gamma, const float* beta,
                        const float* temb, int ldt, const float* residual, void* y, void* y16, int ldy16,
                        float* stats, int io, void* stream);
/* GroupNorm + Mish (+ time bias) (+ residual) as a STREAMING apply fed by the sums the producing conv's epilogue left (mi_conv3x3_pw_gnsums:
 * sums [N][C / 16][2], 64-bit fixed point): no statistics pass, no (sample, group) workgroups -- a workgroup is a run of pixels of one
 * sample x all channels.  Replaces aten::native_group_norm + Mish + the broadcast / residual adds of reference src/models/ddpm.py:112-120,
 * 139-143 where a tile-kernel conv produced x.  x bf16 [N][HW][C]; y bf16 (y_is_bf16) or fp32, residual fp32 (fp32 y only), y_bf16 an
 * optional bf16 copy of an fp32 y, stats [N][G][2] = {mean, rstd} (optional, what the backward pass reads).  Returns 0 when launched,
 * 1 when the shape is not taken (C / G % 16, C / 8 a power of two <= 256, HW a multiple of the pixels per pass, 16-byte aligned rows):
 * the caller then runs mi_gn_mish_fwd_io. */
int mi_gn_mish_apply_sums(const MiGnDesc* d, const void* x, const void* sums, const float* gamma, const float* beta, const float* temb,
                          int ldt, const float* residual, void* y, int y_is_bf16, void* y_bf16, int ldy16, float* stats, void* stream);
/* statistics-only pass for the fused conv above */
int mi_gn_stats_coef(const MiGnDesc* d, const void* x, const float* gamma, const float* beta, const float* temb, int ldt,
                     float* stats, float* coef, int x_is_bf16, void* stream);
int mi_gn_mish_bwd_io(const MiGnDesc* d, const void* x, const float* stats, const float* gamma, const float* beta,
                      const void* dout, int lddo, void* dx, int lddx, float* dgamma, float* dbeta, float* dtemb,
                      int ldt, float* dbias, int io, void* stream);

/* ---- channel LayerNorm (ddpm.py:85-95; eps added to the std) ---------------------------- */
int mi_chan_layernorm_fwd(int M, int C, const float* x, int ldx, const float* g, const float* b,
                          float eps, float* y, int ldy, void* stream);
int mi_chan_layernorm_bwd(int M, int C, const float* x, int ldx, const float* g, float eps,
                          const float* dy, int lddy, float* dx, int lddx, int accumulate_dx,
                          float* dg, float* db, void* stream);
/* the same with the LayerNorm output (y16) / its gradient (dy16) stored as bf16; x and dx stay fp32 */
int mi_chan_layernorm_fwd_io(int M, int C, const float* x, int ldx, const float* g, const float* b,
                             float eps, void* y, int ldy, int y16, void* stream);
int mi_chan_layernorm_bwd_io(int M, int C, const float* x, int ldx, const float* g, float eps,
                             const void* dy, int lddy, float* dx, int lddx, int accumulate_dx,
                             float* dg, float* db, int dy16, void* stream);
/* the same with the parameter gradients left as partial rows: part[r][2 C] = (dg | db) sums of workgroup r for
 * r < mi_chan_layernorm_bwd_part_rows(M, C) (every row is written); mi_rowsum_batch adds them into dg / db */
int mi_chan_layernorm_bwd_part_rows(int M, int C);
int mi_chan_layernorm_bwd_part(int M, int C, const float* x, int ldx, const float* g, float eps,
                               const void* dy, int lddy, float* dx, int lddx, int accumulate_dx,
                               float* part, int dy16, void* stream);
/* out of place: dx_out = dx_in + grad with dx_in read only -- bit for bit what the accumulating in-place call leaves in dx.
 * dx_in == dx_out (same pitch) is that call; any other overlap of the two [M][C] ranges is refused before anything is
 * written.  part != NULL: parameter gradients as partial rows (as _part); else atomics into dg / db (either may be NULL). */
int mi_chan_layernorm_bwd_out(int M, int C, const float* x, int ldx, const float* g, float eps,
                              const void* dy, int lddy, const float* dx_in, int lddx_in, float* dx_out, int lddx_out,
                              float* dg, float* db, float* part, int dy16, void* stream);
/* 1 if the four backward entry points above run these pointers and pitches on the pipelined kernel (C = 128, 256 or 512, x / dx /
 * dx_in 16-byte aligned, dy 8-byte (bf16) or 16-byte aligned: several pixel groups of a wave in flight, the same bits), 0 if on the
 * guarded one.  dx_in: NULL when nothing is accumulated, dx itself for the accumulating in-place calls. */
int mi_chan_layernorm_bwd_pipelined(int C, const void* x, const void* dy, const void* dx, const void* dx_in, int ldx, int lddy,
                                    int lddx, int lddx_in, int dy16);
int mi_debug_ln_bwd_pipeline(int on);           /* tests / A-B switch: 0 = the guarded kernel for every launch, anything else = the pipelined one where it applies (default); returns the previous value (0 or 1) */

/* ---- LinearAttention core (ddpm.py:157-165), heads x 32 channels -------------------------
 * qkv[b][p][3*heads*32] (q | k | v, head-major inside each), out[b][p][heads*32].
 * ctx[b][h][32][32] and kstat[b][h][32][2] = {max, sum exp} are saved for backward. */
int mi_linattn_fwd(int B, int n, int heads, const float* qkv, float* out, float* ctx,
                   float* kstat, void* stream);
int mi_linattn_bwd(int B, int n, int heads, const float* qkv, const float* ctx,
                   const float* kstat, const float* dout, float* dqkv, void* stream);
/* bf16 storage of the attention-internal activations: b16 != 0 -> qkv and out (forward), qkv, dout and dqkv
 * (backward) are bf16 tensors; ctx, kstat and all arithmetic stay fp32. */
int mi_linattn_fwd_io(int B, int n, int heads, const void* qkv, void* out, float* ctx, float* kstat, int b16,
                      void* stream);
int mi_linattn_bwd_io(int B, int n, int heads, const void* qkv, const float* ctx, const float* kstat,
                      const void* dout, void* dqkv, int b16, void* stream);
/* ... with a scratch buffer (mi_linattn_workspace(B, n, heads) bytes, 16-byte aligned; 0 = not needed): images with many pixels per
 * (batch, head) are cut into pixel slices, one workgroup each -- three launches forward (slice max, slice exp / outer product,
 * combine + out), two backward (slice dctx, combine + per-pixel gradients) -- so that every CU holds several workgroups' loads in
 * flight instead of one workgroup walking 1024-4096 pixels.  Partial results are combined in a fixed order (deterministic).  A
 * null / too small workspace runs one workgroup per (batch, head). */
size_t mi_linattn_workspace(int B, int n, int heads);
int mi_linattn_fwd_ws(int B, int n, int heads, const void* qkv, void* out, float* ctx, float* kstat, int b16,
                      void* workspace, size_t ws_bytes, void* stream);
int mi_linattn_bwd_ws(int B, int n, int heads, const void* qkv, const float* ctx, const float* kstat,
                      const void* dout, void* dqkv, int b16, void* workspace, size_t ws_bytes, void* stream);

/* ---- small exact-fp32 GEMM: nn.Linear of the time-embedding MLP (ddpm.py:126-130,186-193), forward, input
 * gradient and weight gradient ---------------------------------------------------------------------
 *   C[i][j] (+)= bias[j] + sum_k opA(i,k) * opB(k,j),   opA = ta ? A[k*lda+i] : A[i*lda+k],  opB = tb ? B[j*ldb+k] : B[k*ldb+j]
 * forward y = x W^T + b: ta 0, tb 1;  dx = dy W: ta 0, tb 0;  dW += dy^T x: ta 1, tb 0, accumulate 1.
 * Needs K % 32 == 0, ld % 4 == 0, 16-byte aligned A / B (mi_small_gemm_supported); with allow_split long contractions are
 * split and combined with fp32 atomics (used for the gradients only: the forward stays bit-reproducible). */
int mi_small_gemm(int ta, int tb, int I, int J, int K, const float* A, int lda, const float* B, int ldb,
                  const float* bias, float* C, int ldc, int accumulate, int allow_split, void* stream);
int mi_small_gemm_supported(int ta, int tb, int I, int J, int K, int lda, int ldb);

/* ---- VQ-VAE codebook step (reference src/models/vqvae.py:24-43) ---------------
 * Forward: for each of the M latent rows z[m][0..D) (row stride ldz) the nearest of the K codebook rows
 * (torch.cdist + argmin: squared distances ||z||^2 + ||e||^2 - 2 z.e on the exact-fp32 matrix cores, lowest
 * index on ties), idx[m], the gathered rows zq[m][0..D), and loss_partial[b] = sum over workgroup b's rows of
 * ||z - zq||^2 (mi_vq_partials(M) floats; vq_loss = sum / (M*D), commit_loss = weight * the same).  D % 4 == 0, D <= 128.
 * Backward of g_vq * mean((sg(z) - q)^2) + g_commit * mean((z - sg(q))^2):
 *   dz (+)= g_commit * 2 (z - q) / (M D)   (dz may be null),   dcodebook[idx[m]] += g_vq * 2 (q - z_m) / (M D);
 * g_dev (nullable) points at two device floats multiplied into (g_vq, g_commit): the upstream loss gradients without a
 * host round trip.  mi_vq_scatter_rows: table[idx[m]] += src[m] -- what the gather `embedding[z_index]` (vqvae.py:37)
 * passes back to the codebook when quant_z itself is differentiated. */
int mi_vq_partials(int M);
int mi_vq_nearest_fwd(int M, int D, int K, const float* z, int ldz, const float* codebook, int* idx, float* zq, int ldq,
                      float* loss_partial, void* stream);
int mi_vq_bwd(int M, int D, int K, const float* z, int ldz, const float* codebook, const int* idx, float g_vq, float g_commit,
              const float* g_dev, float* dz, int lddz, int accumulate_dz, float* dcodebook, void* stream);
int mi_vq_scatter_rows(int M, int D, int K, const float* src, int ld, const int* idx, float* table, void* stream);

/* ---- WGAN-GP operators (reference src/models/wgan_gp.py:62-107, src/networks/basic.py:9-40) -------------
 * Sample norm = nn.GroupNorm(1, C) (`norm_type="layer"`, forced at wgan_gp.py:30-31) on dense NHWC tensors [N][P][C],
 * C % 4 == 0 and 2048 % C == 0; stats = [N][2] (mean, rstd).
 *   fwd : y = gamma (x - mean) rstd + beta
 *   bwd : dx = dL/dx (+ extra_dx when non-null; dx may alias dy); dgamma, dbeta accumulated (nullable)
 *   bwd2: the backward of bwd, for the gradient penalty's create_graph=True (wgan_gp.py:89-96): given the adjoint u of dx,
 *         adj_dy = d<u,dx>/d dy, adj_x = d<u,dx>/d x, dgamma += d<u,dx>/d gamma. */
int mi_sample_norm_supported(int N, int P, int C);
int mi_sample_norm_fwd(int N, int P, int C, const float* x, const float* gamma, const float* beta, float* y, float* stats, float eps,
                       void* stream);
int mi_sample_norm_bwd(int N, int P, int C, const float* x, const float* stats, const float* gamma, const float* dy, const float* extra_dx,
                       float* dx, float* dgamma, float* dbeta, void* stream);
int mi_sample_norm_bwd2(int N, int P, int C, const float* x, const float* stats, const float* gamma, const float* dy, const float* u,
                        float* adj_dy, float* adj_x, float* dgamma, void* stream);
/* LeakyReLU(slope) / Tanh on dense vectors (n % 4 == 0); backward from the OUTPUT y; in-place allowed (y == x, dx == dy). */
int mi_leaky_relu_fwd(size_t n, const float* x, float* y, float slope, void* stream);
int mi_leaky_relu_bwd(size_t n, const float* y, const float* dy, float* dx, float slope, void* stream);
int mi_tanh_fwd(size_t n, const float* x, float* y, void* stream);
int mi_tanh_bwd(size_t n, const float* y, const float* dy, float* dx, void* stream);
/* out[s][i] = e[s] a[s][i] + (1 - e[s]) b[s][i], s < N, i < per (wgan_gp.py:84-87) */
int mi_lerp_rows(int N, size_t per, const float* a, const float* b, const float* e, float* out, void* stream);
/* gradient penalty (wgan_gp.py:95-97): *penalty += mean_s (||g_s||_2 - 1)^2 (nullable) and, when u is non-null,
 * u_s = scale * (scale_dev ? *scale_dev : 1) * d penalty / d g_s. */
int mi_gp_penalty(int N, size_t per, const float* g, float* penalty, float* u, float scale, const float* scale_dev, void* stream);

/* ---- VAE operators (BASELINE cfg 1; reference src/models/vae.py:46-72, src/networks/basic.py:147-204, src/utils/losses.py:30-32) ----
 * nn.BatchNorm2d on a dense NHWC tensor of M = N*H*W rows and C channels (C % 4 == 0, C/4 a power of two <= 256).
 * training != 0: batch statistics (left in mean / rstd for the backward), running statistics updated like torch (momentum,
 * unbiased variance) when non-null; training == 0: mean / rstd come from the running statistics.
 * ws: mi_batchnorm_workspace(C) bytes, zero on entry, left zero on exit.  bwd: dx may alias dy, dgamma / dbeta accumulated. */
int mi_batchnorm_workspace(int C);
int mi_batchnorm_fwd(int M, int C, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                     float* running_mean, float* running_var, float momentum, float eps, int training, void* ws, void* stream);
int mi_batchnorm_bwd(int M, int C, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dy,
                     float* dx, float* dgamma, float* dbeta, void* ws, void* stream);
/* latent block: h = [mu | log_sigma] (rows of ldh >= 2L floats), z = mu + exp(log_sigma) * eps (vae.py:46-55, eps drawn by the
 * caller), *kld += mean over rows of -0.5 sum(1 + 2 log_sigma - mu^2 - exp(2 log_sigma)) (losses.py:30-32; nullable).
 * bwd: dh = dL/dh from dz = dL/dz and g_kld * (g_dev ? *g_dev : 1) = dL/d kld. */
int mi_vae_latent_fwd(int N, int L, const float* h, int ldh, const float* eps, float* z, float* kld, void* stream);
int mi_vae_latent_bwd(int N, int L, const float* h, int ldh, const float* eps, const float* dz, float g_kld, const float* g_dev,
                      float* dh, int lddh, void* stream);

/* ---- cVAE operators (reference src/models/cvae.py; csrc/cvae_ops.hip) ------------------------------------------------------------
 * Label-indexed data movement of the label-conditioned VAE; labels are int64[N] on the device.  fp32, no atomics: every sum has
 * a fixed order, so two calls on the same inputs give the same bits.  A label outside [0, ncls) selects nothing (no one-hot
 * plane, a zero embedding half, no gradient row) and is never used as an index.
 * mi_cvae_pack_input: NCHW images -> the encoder's NHWC input [N][HW][ld], ld >= C + ncls: channels < C the image, channel C + k
 *   1 where k == labels[n] else 0, channels >= C + ncls zero (cvae.py:66-69 without the one-hot tensor).  Every element is stored.
 * mi_cvae_latent_fwd: h = [mu | log_sigma] (rows of ldh >= 2L), E = class_embedding.weight [ncls][L];
 *   zc[n] = [mu + exp(log_sigma) eps | E[labels[n]]] (dense rows of 2L; the embedding half is a copy), *kld = the KL term of
 *   mi_vae_latent_fwd, STORED by one workgroup (nullable).  h == null: zc[n] = [eps[n] | E[labels[n]]] -- eps holds z, the decode
 *   path of forward(z, labels) (cvae.py:43-46); kld must be null then.
 * mi_cvae_latent_bwd: dzc = dL/dzc (rows of lddzc >= 2L); dh (dense [N][2L]) = what mi_vae_latent_bwd gives for dz = dzc[:, :L];
 *   dE[c][j] += sum over the rows n with labels[n] == c, in ascending n, of dzc[n][L + j]; rows of dE whose class no row carries
 *   are neither read nor written. */
int mi_cvae_pack_input(int N, int C, int HW, int ncls, const float* x_nchw, const int64_t* labels, float* y_nhwc, int ld, void* stream);
int mi_cvae_latent_fwd(int N, int L, int ncls, const float* h, int ldh, const float* eps, const int64_t* labels, const float* E,
                       float* zc, float* kld, void* stream);
int mi_cvae_latent_bwd(int N, int L, int ncls, const float* h, int ldh, const float* eps, const int64_t* labels, const float* dzc,
                       int lddzc, float g_kld, const float* g_dev, float* dh, float* dE, void* stream);

/* ---- latent discriminator (reference src/networks/basic.py:64-112 as src/models/factor_vae.py:48 builds it; csrc/latent_disc.hip) ----
 * MLPEncoder(L, [256, 256], 1): x [N][L] -> Linear(L,256) -> GroupNorm(1,256) -> LeakyReLU(0.2) -> Linear(256,256) -> BatchNorm1d(256)
 * -> LeakyReLU(0.2) -> Linear(256,1) = logit[N], with the least-squares loss mean((logit - target)^2).  fp32 in every compute mode; no
 * atomics, every sum has a fixed order; every element of every output is stored.  2 launches forward, 3 backward (2 without
 * parameter gradients).
 * supported: 1 for H == 256, 1 <= L <= 64, 2 <= N <= MI_LATENT_DISC_NMAX, else 0 with a message in mi_last_error().  N == 1 is refused
 *   because BatchNorm1d has no batch statistics there; NMAX because the forward's tail is ONE workgroup that keeps the N logits in LDS
 *   (4 B each) and walks the rows serially -- a wider batch wants that tail split, which is not built.
 * params / grads: host arrays of 10 device pointers: fc1.weight [L][256] (input-major), fc1.bias, norm1.weight, norm1.bias,
 *   fc2.weight [256 in][256 out], fc2.bias, norm2.weight, norm2.bias, fc3.weight [256], fc3.bias [1].
 * input, one of: z (rows of ldz >= L; h, eps, perm null) | h = [mu | log_sigma] (rows of ldh >= 2L) + eps [N][L]: x = mu + exp(log_sigma) eps
 *   formed on the fly | the same + perm int64 [L][N]: x[n][j] = z[perm[j][n]][j] (factor_vae.py:13-22).  A perm entry outside [0, N)
 *   makes that element 0 and is never used as an address.
 * fwd: tape (mi_latent_disc_tape_floats(N) floats, 16-byte aligned) = xhat1 [N][256] | h1 [N][256] | a2 [N][256] | LayerNorm (mean, rstd) [N][2]
 *   | BatchNorm (mean, rstd) [2][256] as fp64 (1024 floats) | logit [N].  Tensors are fp32, sums and BatchNorm's arithmetic fp64;  out3[0] = loss, out3[1] = mean(logit), out3[2] = mean(logit^2) (the loss against target 0).  training != 0: batch statistics, and
 *   running_mean / running_var (nullable pair; momentum, unbiased variance) and *num_batches_tracked (nullable, += 1) are updated;
 *   training == 0: the running statistics normalise.
 * bwd: of the loss against `target` (which may differ from the forward's: the tape does not depend on it), with the forward's input
 *   and mode.  grads (nullable): g = (accumulate_params ? g : 0) + param_scale * dloss/dparam;  dz (nullable, rows of lddz >= L, not
 *   with perm): dz = (accumulate_dz ? dz : 0) + dz_scale * dloss/dx.  workspace: mi_latent_disc_workspace_floats(N) floats. */
#define MI_LATENT_DISC_NMAX 1024
int mi_latent_disc_supported(int N, int L, int H);
size_t mi_latent_disc_tape_floats(int N);
size_t mi_latent_disc_workspace_floats(int N);
int mi_latent_disc_fwd(int N, int L, int H, const float* z, int ldz, const float* h, int ldh, const float* eps, const int64_t* perm,
                       const float* const* params, int training, float target, float momentum, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, float* tape, float* out3, void* stream);
int mi_latent_disc_bwd(int N, int L, int H, const float* z, int ldz, const float* h, int ldh, const float* eps, const int64_t* perm,
                       const float* const* params, int training, float target, const float* tape, float* workspace, float* const* grads,
                       float param_scale, int accumulate_params, float* dz, int lddz, float dz_scale, int accumulate_dz, void* stream);

/* ---- row-local latent discriminator (reference src/models/aae.py:42-44: MLPEncoder(L, [256, 256], 1, norm_type="layer");
 *      csrc/latent_disc_ln.hip) ----
 * x [N][L] -> Linear(L,256) -> GroupNorm(1,256) -> LeakyReLU(0.2) -> Linear(256,256) -> GroupNorm(1,256) -> LeakyReLU(0.2) -> Linear(256,1)
 * = logit[N].  No batch statistics: a row's logit depends on that row alone, so N = 1 is legal and the batch may be two SEGMENTS with a
 * target each -- rows [0, N0) from x0 (rows of ld0 >= L) against target0, rows [N0, N0 + N1) from x1 (rows of ld1 >= L) against target1;
 * N1 = 0 is allowed (x1 is not read).  The logits of a joint pass equal those of the two separate passes bit for bit.
 * loss per row, loss_mode 0 (vanilla, binary cross-entropy on the logit): max(x, 0) - x t + log1p(exp(-|x|)), derivative sigmoid(x) - t;
 *   loss_mode 1 (lsgan): (x - t)^2.
 * fp32 in every compute mode, sums in fp64 in a fixed order; no atomics; every element of every output is stored.  2 launches forward,
 * 2 backward, 1 backward when only the input gradient is asked for.
 * supported: 1 for H == 256, 1 <= L <= 64, N0 >= 1, N1 >= 0, N0 + N1 <= MI_LATENT_DISC_LN_NMAX, else 0 with a message in mi_last_error().
 *   NMAX: the parameter-gradient sums walk the N0 + N1 rows serially in 34 + ceil(L/8) workgroups; a wider batch wants them split.
 * params / grads: the ten pointers of mi_latent_disc_fwd in the same order and layout (norm2 is the second GroupNorm's affine pair).
 * fwd: tape (mi_latent_disc_ln_tape_floats(N0 + N1) floats, 16-byte aligned) = xhat1 [N][256] | h1 [N][256] | xhat2 [N][256] | rstd1 [N]
 *   | rstd2 [N] | logit [N] | loss per row [N].  out5 = loss0, loss1 (each the mean over its own segment), mean(logit) of segment 0, of
 *   segment 1, 0.5 (loss0 + loss1); an empty second segment gives loss1 = mean1 = 0.
 * bwd: of c0 loss0 + c1 loss1 against target0 / target1 (which may differ from the forward's: the tape holds no target-dependent
 *   value but the per-row loss, which the backward does not read), with the forward's inputs.  grads (nullable; needs workspace,
 *   mi_latent_disc_ln_workspace_floats(N0 + N1) floats): g = (accumulate_params ? g : 0) + param_scale * d/dparam.  dx0 (nullable; N0 rows
 *   of lddx >= L, the first segment's input gradient): dx0 = (accumulate_dx ? dx0 : 0) + dx_scale * d/dx0; lanes [L, lddx) are not written. */
#define MI_LATENT_DISC_LN_NMAX 65536
int mi_latent_disc_ln_supported(int N0, int N1, int L, int H);
size_t mi_latent_disc_ln_tape_floats(int N);
size_t mi_latent_disc_ln_workspace_floats(int N);
int mi_latent_disc_ln_fwd(int N0, int N1, int L, int H, const float* x0, int ld0, const float* x1, int ld1, const float* const* params,
                          int loss_mode, float target0, float target1, float* tape, float* out5, void* stream);
int mi_latent_disc_ln_bwd(int N0, int N1, int L, int H, const float* x0, int ld0, const float* x1, int ld1, const float* const* params,
                          int loss_mode, float target0, float target1, float c0, float c1, const float* tape, float* workspace,
                          float* const* grads, float param_scale, int accumulate_params, float* dx0, int lddx, float dx_scale,
                          int accumulate_dx, void* stream);

/* ---- plain GAN (reference src/models/gan.py, src/utils/losses.py:4-24): segmented BatchNorm + activation, adversarial losses ----
 * x: dense NHWC rows [S*M][C] fp32, S >= 1 segments of M rows each; C as mi_batchnorm_fwd (C % 4 == 0, C/4 a power of two <= 256).
 * act: 0 none, 1 ReLU, 2 LeakyReLU(slope).  Two launches each way: per-workgroup fp64 partial sums STORED into a workspace slot per
 * (segment, workgroup), then an apply pass whose workgroups add their channels' partials in a fixed order and stream the tensor.  No
 * atomics, no zero-on-entry workspace, no grid sync: two runs give the same bits.  ws: mi_bn_seg_workspace(S, M, C) bytes, 8-byte
 * aligned, any content.  mi_bn_seg_rows_per_workgroup(M, C): the rows one sums workgroup walks (a function of M and C alone).
 * fwd, training != 0: y = act(gamma (x - mean_s) rstd_s + beta) with the mean and biased variance of segment s; mean / rstd [S][C] are
 *   left for the backward; running statistics (nullable) take the S updates in segment order, s = 0 first (torch's momentum rule,
 *   unbiased variance, M == 1: the biased one), one thread per channel.  training == 0: every segment uses the running statistics.
 *   y must not alias x.
 * bwd (of the training-mode forward): g = act'(y) dy from the activated OUTPUT y (the convention of mi_leaky_relu_bwd), never written;
 *   dx = gamma rstd_s (g - S0_s / M - xhat S1_s / M), dx may alias dy; dgamma = sum_s S1_s, dbeta = sum_s S0_s (nullable), stored
 *   (accumulate == 0) or added (accumulate != 0). */
size_t mi_bn_seg_workspace(int S, int M, int C);
int mi_bn_seg_rows_per_workgroup(int M, int C);
int mi_bn_seg_fwd(int S, int M, int C, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                  float* running_mean, float* running_var, float momentum, float eps, int training, int act, float slope, void* ws,
                  void* stream);
int mi_bn_seg_bwd(int S, int M, int C, const float* x, const float* mean, const float* rstd, const float* gamma, const float* y,
                  const float* dy, float* dx, float* dgamma, float* dbeta, int accumulate, int act, float slope, void* ws, void* stream);
/* logit: S <= 8 segments of M logits, ld floats apart (dlogit: lddl); target_is_real: S ints on the HOST, read before the call returns.  One launch, one
 * workgroup, fp64 sums in a fixed order.  loss[S] = mean loss of the segment, mean_logit[S], dlogit[S*M] (nullable) =
 * scale * d loss_s / d logit.  mode 0 vanilla: BCE with logits, max(-+x, 0) + log1p(exp(-|x|)), finite at |x| = 200;  1 lsgan:
 * (x - t)^2, t = 1 | 0;  2 hinge AS THE REFERENCE COMPUTES IT: real max(1 - x, 1), fake max(1 + x, 0) -- the real branch is not the
 * textbook hinge max(1 - x, 0); a tie of the two operands halves the gradient, as torch.maximum does;  3 wasserstein (the WGAN critic,
 * wgan.py:70-90): -x for a real segment, +x for a fake one, dlogit = -+scale / M. */
int mi_adv_loss(int S, int M, int mode, const int* target_is_real, float scale, const float* logit, int ld, float* loss,
                float* mean_logit, float* dlogit, int lddl, void* stream);

/* ---- InfoGAN heads and latent packing (reference src/models/info_gan.py:37-43, 64-133; csrc/info_head.hip) ----
 * The heads sit on the shared feature f [S*M][E] (rows of ldf >= E floats: the common layer's NHWC output, read in place), S <= 2 segments:
 *   a = LeakyReLU(f, 0.01) (torch's default slope; never stored), logit = a w_d + b_d, q1 = LeakyReLU(a W1 + b1, 0.01) [rows][128],
 *   q = q1 W2 + b2 [rows][Qd], Qd = Dd V + Cc.  q's first Dd V columns are [V][Dd]: value v of code d is column v Dd + d, the layout of the
 *   reference's flattened [N, V, Dd] one-hot; the last Cc columns are the continuous codes.
 * params / grads: six pointers w_d [E], b_d [1], W1 [E][128], b1 [128], W2 [128][Qd], b2 [Qd] (weights input-major; W1 16-byte aligned).
 * fp32 tensors, every sum fp64 in a fixed order and rounded once, no atomics, every element of every output stored, the workspace needs
 * no zeroing: two runs agree bit for bit.  2 launches forward; backward 2, 1 without parameter gradients.
 * supported: 1 for Hd == 128, E % 4 == 0, 4 <= E <= 4096, S in {1, 2}, M >= 1 and either Dd = V = Cc = 0 (the D head alone) or Dd, V,
 *   Cc >= 1 with Dd V + Cc <= 64; else 0 with a message in mi_last_error().
 * mi_info_latent: out [N][ld] = [ones at v Dd + d for v = dis_c_index[n][d] | cont_c [N][Cc] | z [N][Nz] | 0 up to ld], one launch, every
 *   element written.  An index outside [0, V) is not detected (that would cost a host synchronisation): its code's V columns stay 0.
 * fwd: the D head is computed iff logit is non-null (then params[0..1], dlogit, ws and out6 are needed; else dlogit is null too).
 *   The Q head is computed iff q is non-null (params[2..5]); with dis_c_index [rows][Dd] also its losses (then cont_c (rows of ldc), q1,
 *   dq, ws and out6 are needed).  With dis_c_index, cont_c and dq all null it is the Q head's output alone: q, and q1 unless null, for
 *   Qd = Dd V + Cc in [1, 64] (Dd = V = 0, Cc = Qd will do), one launch when there is no D head either.
 *   The adversarial loss is binary cross-entropy with logits (mi_adv_loss mode 0, the same stable form) against target{0,1}_is_real
 *   per segment.  dlogit [rows] = scale / M * d loss_s / d logit;  dq [rows][Qd] = lambda_I * d (I_disc + I_cont) / dq with I_disc the
 *   cross-entropy of the Dd softmaxes over V averaged over rows * Dd, I_cont the squared error averaged over rows * Cc.
 *   ws: mi_info_head_workspace_doubles(rows) doubles.  out6 = loss of segment 0, of segment 1, mean logit of segment 0, of segment 1,
 *   I_disc, I_cont (0 for what was not computed).
 * bwd: from f, q1, dlogit and dq (null: the D head alone).  df (nullable, rows of lddf >= E) = leaky'(f) (dlogit w_d + (leaky'(q1) (dq W2^T)) W1^T).
 *   grads (nullable array; each group all set or all null): [2..5] the Q gradients (need dq and dq1_ws, rows * 128 floats),
 *   [0..1] the D-head gradients.  Gradients are stored, never accumulated. */
int mi_info_latent(int N, int Dd, int V, int Cc, int Nz, const long long* dis_c_index, const float* cont_c, int ldc, const float* z, int ldz,
                   float* out, int ld, void* stream);
int mi_info_head_supported(int S, int M, int E, int Hd, int Dd, int V, int Cc);
size_t mi_info_head_workspace_doubles(int rows);
int mi_info_head_fwd(int S, int M, int E, int Hd, const float* f, int ldf, const float* const* params, int target0_is_real,
                     int target1_is_real, float scale, int Dd, int V, int Cc, const long long* dis_c_index, const float* cont_c, int ldc,
                     float lambda_I, float* logit, float* dlogit, float* q1, float* q, float* dq, double* ws, float* out6, void* stream);
int mi_info_head_bwd(int S, int M, int E, int Hd, int Qd, const float* f, int ldf, const float* const* params, const float* dlogit,
                     const float* q1, const float* dq, float* df, int lddf, float* dq1_ws, float* const* grads, void* stream);

/* ---- AGE latent moments (reference src/models/age.py:64-81, 90-144; csrc/age_ops.hip) ----
 * The code buffer e holds S <= 2 segments of M rows, L <= 512 columns, rows of ld >= L floats (the encoder's NHWC output, read in
 * place; any pitch, no alignment assumed; columns from L on are never read).
 * fp32 tensors, every sum fp64 in a fixed order and rounded once, no atomics, every element of every output stored, the workspace
 * needs no zeroing: two runs agree bit for bit.
 * supported: 1 for S in {1, 2}, M >= 2 (the unbiased variance), 1 <= L <= 512; else 0 with a message in mi_last_error().
 * fwd: normalize != 0: z [S*M][L] (dense) = e / max(||e||_2, 1e-12) per row (F.normalize) and norm [S*M] = ||e||_2; else z = e and both
 *   pointers are null.  want_stats != 0: per segment mu [S][L], var [S][L] (unbiased, over the segment's rows of z) and
 *   out4 [S][4] = kl = mean_j (mu_j^2 + var_j - log var_j) / 2, mean_j mu_j, mean_j var_j, the reconstruction loss of mode_s against the
 *   target rows t [M][L] (rows of ldt; both segments read the same M rows): mode 0 none (stored as 0), 1: 1 - mean_i cos(z_i, t_i) as
 *   torch's cosine_similarity computes it (each row divided by its norm clamped at 1e-8), 2: mean_ij (z_ij - t_ij)^2.
 *   ws: mi_age_moments_workspace_doubles(S, M) doubles, needed with a mode.  2 launches; 1 without normalisation and modes, and 1
 *   with want_stats == 0 (the normalisation alone: the prior draw; then M >= 1 is accepted and mu, var, out4 are null).
 * bwd: one launch.  z (rows of ldz) and norm as the forward stored them, or z = e and norm = null without normalisation.
 *   g_ij = c_s / L (mu_j / M + (1 - 1 / var_j) (z_ij - mu_j) / (M - 1)) + w_s d recon_s / d z_ij + dz_ext_s[i][j]
 *   (dz_ext_s [M][L], rows of ldx, nullable);  de = (g - z (z . g)) / norm for norm >= 1e-12 and g / 1e-12 below (clamp_min's
 *   derivative), de = g without normalisation.  de [S*M][ldde]: every element stored, columns from L on as 0. */
/* mi_age_image_mse: the AGE's image reconstruction term F.mse_loss(imgs, decoder(real_z)) (age.py:109, 142) with its gradient, 2 launches:
 *   loss[0] = mean (pred - target)^2 over B C HW (stored, not accumulated), pred NHWC with pixel pitch ld, target NCHW;
 *   dpred [B*HW][ld] (nullable) = gscale * 2 (pred - target) / (B C HW), lanes from C on stored as 0.  As mi_eps_loss with loss_type 1,
 *   but the workgroups' fp64 sums go to ws (mi_age_image_mse_workspace_doubles(B, HW) doubles, no zeroing) and are added in a fixed
 *   order: the loss has the same bits on every run. */
size_t mi_age_image_mse_workspace_doubles(int B, int HW);
int mi_age_image_mse(int B, int C, int HW, const float* pred, int ld, const float* target, float* loss, float* dpred, float gscale,
                     double* ws, void* stream);
int mi_age_moments_supported(int S, int M, int L);
size_t mi_age_moments_workspace_doubles(int S, int M);
int mi_age_moments_fwd(int S, int M, int L, const float* e, int ld, int normalize, float* z, float* norm, int want_stats, int mode0,
                       int mode1, const float* t, int ldt, float* mu, float* var, float* out4, double* ws, void* stream);
int mi_age_moments_bwd(int S, int M, int L, const float* z, int ldz, const float* norm, const float* mu, const float* var, float c0,
                       float c1, int mode0, int mode1, float w0, float w1, const float* t, int ldt, const float* dz_ext0,
                       const float* dz_ext1, int ldx, float* de, int ldde, void* stream);

/* ---- VAE-GAN operators (reference src/models/vae_gan.py:63-102; csrc/vaegan_ops.hip) ----
 * fp32 tensors, every sum fp64 in a fixed order and rounded once, no atomics, every element of every output stored (pad lanes as 0),
 * the workspace needs no zeroing: two runs agree bit for bit.  Output rows have pitches that are multiples of 4 floats and 16-byte
 * aligned bases: every store is a 16-byte access.  A refused call returns non-zero with mi_last_error() set and writes nothing.
 * latent_supported: 1 for N >= 1, L >= 1, N (L + 3) < 2^27, else 0 with a message.
 * latent_fwd: h [N][ldh >= 2L] = [mu | log_sigma], eps [N][L], prior [N][L] (dense) -> z [2N][ldz], ldz = 4 ceil(L / 4): rows [0, N) =
 *   mu + exp(log_sigma) eps, rows [N, 2N) = prior, lanes from L on 0 -- the decoder's NHWC input for one segments=2 pass.  kld[0] is
 *   STORED: mean over rows of -0.5 sum(1 + 2 ls - mu^2 - exp(ls)^2), each term as mi_vae_latent_fwd forms it, summed in fp64.  1 launch.
 * latent_bwd: dh [N][lddh], lddh = 4 ceil(2L / 4): lanes [0, L) = d + gk mu, [L, 2L) = d eps exp(ls) + gk (exp(ls)^2 - 1), the rest 0,
 *   with d = dz_scale * dz[n][k] (dz: the first N rows of the decoder's input gradient, rows of lddz >= L) and gk = g_kld / N.  1 launch.
 * feat_match: real, recon: two dense 16-byte aligned blocks of N * per floats (per % 4 == 0; two segments of netD's last hidden NHWC
 *   activation, read in place).  loss[0] = sum (real - recon)^2 / N, stored.  drecon (nullable, may be a segment of a larger buffer) =
 *   gscale * 2 (recon - real) / N, stored (accumulate == 0) or added.  ws: mi_feat_match_workspace_doubles(N, per) doubles.  2 launches.
 * pack_fwd: dec_out [2N][HW][ld] = the decoder's [recon | fake] output and the NCHW batch -> x [3N][HW][ld] = [fake | nhwc(imgs) | recon],
 *   ld % 4 == 0, ld >= C, lanes from C on 0.  unpack_bwd: dx [3N][HW][ld] (netD's input gradient) -> dy [2N][HW][ld] =
 *   [s_recon dx[2N:3N] | s_fake dx[0:N]], lanes from C on 0.  1 launch each; 3 N HW ld < 2^31. */
int mi_vaegan_latent_supported(int N, int L);
int mi_vaegan_latent_fwd(int N, int L, const float* h, int ldh, const float* eps, const float* prior, float* z, int ldz, float* kld,
                         void* stream);
int mi_vaegan_latent_bwd(int N, int L, const float* h, int ldh, const float* eps, const float* dz, int lddz, float dz_scale, float g_kld,
                         float* dh, int lddh, void* stream);
int mi_feat_match_supported(int N, int per);
size_t mi_feat_match_workspace_doubles(int N, int per);
int mi_feat_match(int N, int per, const float* real, const float* recon, float* loss, float* drecon, float gscale, int accumulate,
                  double* ws, void* stream);
int mi_vaegan_pack_supported(int N, int C, int HW, int ld);
int mi_vaegan_pack_fwd(int N, int C, int HW, const float* dec_out, const float* imgs_nchw, float* x, int ld, void* stream);
int mi_vaegan_unpack_bwd(int N, int C, int HW, const float* dx, float s_recon, float s_fake, float* dy, int ld, void* stream);

/* ---- small element-wise pieces ---------------------------------------------------------------- */
/* SinusoidalPosEmb (ddpm.py:52-59): out[b][dim] = [sin(t f_j) | cos(t f_j)] */
int mi_time_embed(int B, int dim, const int64_t* t, float* out, void* stream);
/* Mish on a flat vector (ddpm.py:62-64) and its backward */
int mi_mish_fwd(size_t n, const float* x, float* y, void* stream);
int mi_mish_bwd(size_t n, const float* x, const float* dy, float* dx, void* stream);
/* ReLU on a flat (dense) vector: y = max(x, 0), y may alias x (nn.ReLU(True), src/networks/vqvae.py:16-20,48,76);
 * backward from the OUTPUT: dx (+)= y > 0 ? dy : 0, dx may alias dy.  16-byte aligned pointers. */
int mi_relu_fwd(size_t n, const float* x, float* y, void* stream);
int mi_relu_bwd(size_t n, const float* y, const float* dy, float* dx, int accumulate, void* stream);
/* NCHW <-> NHWC(ld) */
int mi_nchw_to_nhwc(int B, int C, int HW, const float* x, float* y, int ld, void* stream);
int mi_nhwc_to_nchw(int B, int C, int HW, const float* x, int ld, float* y, void* stream);
/* q_sample (ddpm.py:433-444): x_t = a[t] x0 + b[t] eps ; NCHW in, NHWC(ld) out (+NCHW copy if non-null) */
int mi_q_sample(int B, int C, int HW, const float* x0, const float* noise, const int64_t* t,
                const float* sqrt_ac, const float* sqrt_1mac, float* xt_nhwc, int ld,
                float* xt_nchw, void* stream);
/* loss (ddpm.py:453-456): loss_type 0 = L1 mean, 1 = L2 mean.  pred NHWC(ld), target NCHW.
 * *loss is accumulated (zero it first); dpred (NHWC, may be null) = d loss / d pred * gscale */
int mi_eps_loss(int B, int C, int HW, const float* pred, int ld, const float* target, int loss_type,
                float* loss, float* dpred, float gscale, void* stream);
/* p_sample posterior update (ddpm.py:359-397), x and z NCHW, eps_hat NHWC(ld);
 * writes x_{t-1} NCHW and (if non-null) its NHWC(ldo) copy for the next UNet call. */
int mi_p_sample_update(int B, int C, int HW, const float* x, const float* eps_hat, int ld,
                       const float* z, const int64_t* t, const float* sqrt_recip_ac,
                       const float* sqrt_recipm1_ac, const float* coef1, const float* coef2,
                       const float* logvar, int clip, float* x_prev, float* x_prev_nhwc, int ldo,
                       void* stream);
/* Adam (torch.optim.Adam defaults, ddpm.py:507-511) over one flat buffer.
 * bc1 = 1-b1^step, bc2 = 1-b2^step; grad is multiplied by gscale first (DDP average). */
int mi_adam_step(size_t n, float* p, const float* g, float* m, float* v, float lr, float b1,
                 float b2, float eps, float bc1, float bc2, float gscale, void* stream);
/* mi_adam_step with the complements c1 = 1 - b1 and c2 = 1 - b2 formed by the caller in double and rounded once, as torch's own scalars
 * are (mi_adam_step forms them in fp32: 1.f - 0.999f is off by 4.7e-5, every update by 2.3e-5).  The AGE's optimizers use it. */
int mi_adam_step_c(size_t n, float* p, const float* g, float* m, float* v, float lr, float b2, float c1, float c2, float eps, float bc1,
                   float bc2, float gscale, void* stream);
/* torch.optim.RMSprop with its defaults (no momentum, not centered, no weight decay; wgan.py:50-55) over one flat buffer, one launch:
 * gr = gscale * g;  v = alpha * v + (1 - alpha) * gr^2;  p -= lr * gr / (sqrt(v) + eps).  An element with g = 0 and v = 0 does not move
 * (alignment padding, pad lanes).  p, g, v: 16-byte aligned. */
int mi_rmsprop_step(size_t n, float* p, const float* g, float* v, float lr, float alpha, float eps, float gscale, void* stream);
/* torch.clamp_(lo, hi) in place over n floats, one launch (the WGAN critic's weight clip, wgan.py:67-68).  Written with comparisons:
 * NaN stays NaN, -0.0 stays -0.0, +-inf go to the bounds.  lo <= hi; p may be any float-aligned sub-range of a buffer. */
int mi_clamp_inplace(size_t n, float* p, float lo, float hi, void* stream);
/* The same update with its step count and learning rate in device memory (state[0] = steps taken, stored as the bits of a
 * uint32; state[1] = lr as float), so that a captured hipGraph of forward + backward + optimizer step replays correctly:
 * mi_adam_tick increments state[0] (call it once per optimizer step, before the update of every buffer of that step); the bias
 * corrections 1 - b^state[0] are evaluated in double from the double betas, as the host does for mi_adam_step. */
int mi_adam_tick(float* state, void* stream);
int mi_adam_step_dev(size_t n, float* p, const float* g, float* m, float* v, const float* state, double b1, double b2,
                     float eps, float gscale, void* stream);
/* Device-resident data path: gather B images out of a uint8 dataset [N][H][W][C] that lives in HBM and apply the reference's
 * transform chain (ToTensor, optional per-sample horizontal flip, optional Normalize(0.5, 0.5); reference
 * src/datamodules/base.py:37-71) in torch's own fp32 operation order (u/255, then (v-0.5)/0.5): NCHW fp32 out.
 * idx: int64[B] rows of the dataset; flip: uint8[B] or null. */
int mi_u8_gather_normalize(int B, int C, int H, int W, const uint8_t* data, const int64_t* idx, const uint8_t* flip,
                           int normalize, float* out_nchw, void* stream);
/* fp32 [M][C] (row stride ldx) -> bf16 [M][C] (row stride ldy), round-to-nearest-even: the bf16 copy of a residual-stream tensor
 * that the next layer's conv / weight-gradient kernels read as their MFMA operand (C, ldx, ldy % 4 == 0). */
int mi_f32_to_bf16(size_t M, int C, const float* x, int ldx, void* y_bf16, int ldy, void* stream);
/* y = a*x + (accumulate ? y : 0) */
int mi_axpby(size_t n, float a, const float* x, int accumulate, float* y, void* stream);
/* same on M rows of C channels with row strides (gradient accumulation into channel slices) */
int mi_axpby2d(int M, int C, float a, const float* x, int ldx, int accumulate, float* y, int ldy, void* stream);
/* out[b][0..C) = table[idx[b]][0..C): per-sample rows of a precomputed table (the sampler's time-bias table) */
int mi_gather_rows(int B, int C, const float* table, const int64_t* idx, float* out, void* stream);
/* x[m*ld + c] *= *scalar (scalar lives on the device: autograd's incoming d(loss), no host sync) */
int mi_scale_by_device_scalar(int M, int C, float* x, int ld, const float* scalar, void* stream);

/* ---- PixelCNN operators (reference src/models/pixelcnn.py; csrc/pixelcnn.hip) ------------------------------------------------
 * Masked dilated convolution as an implicit GEMM over the LIVE taps only (masked taps are never read): output pixel (y, x) of
 * column o = sum over taps t and source channels c of x[y + tap_dy[t]][x + tap_dx[t]][c] * w[c*w_sk + o*w_sc + tap_w[t]]
 * (zero outside the image), plus, when C2 > 0, sum over c2 of x2[y][x][c2] * w2[c2*w2_sk + o*w2_sc] (the 1x1 conv1x1_1 of the
 * horizontal stack folded into the same contraction), plus bias[o] + bias2[o] (nullable).  Forward: w_sk = KH*KW, w_sc = Cin*KH*KW
 * on a PyTorch [Cout][Cin][KH][KW] weight; data gradient: the same call with the strides swapped and the offsets negated.
 * elu_in: the x operand goes through ELU on load (the output head).  Epilogues:
 *   MI_PCNN_EPI_PLAIN    y[p][o] = r (+ res[p][o]) (+ y[p][o] when accumulate)
 *   MI_PCNN_EPI_GATE_TS  Cout = 2 gate_C: pre[p][o] = r (raw), y[p][c] = tanh(r_c + cond[n][c]) * sigmoid(r_{C+c} + cond[n][C+c])
 *   MI_PCNN_EPI_GATE_TT  the same with tanh * tanh (the horizontal stack); cond (per-sample bias, row stride ldcond) nullable
 *   MI_PCNN_EPI_ELU_GRAD y[p][o] = (r + res) * elu'(aux[p][o])
 * Both GEMMs run on the matrix cores (desc mode).  The head and the sampling step stay fp32 in both modes (their softmax / log-sum-exp).
 * mi_pcnn_head_supported: Cc 1..4 and the head's LDS staging within 64 KB (Ch <= 254).
 * mi_pcnn_wgrad: dw[c*w_sk + o*w_sc + tap_w[t]] += sum_p x[p + off_t][c] * dy[p][o] (Cin rows, Cout columns; atomics: zero dw first).
 * mi_pcnn_colsum: out[o] (and out2[o], nullable) += sum of column o of g [M][C] (bias gradients; atomics).
 * mi_pcnn_gate_bwd: kind = MI_PCNN_EPI_GATE_TS / _TT; d pre [N*HW][2C] from the raw pre-activations (+ cond) and d out [N*HW][C];
 *   dcond (nullable, row stride ldcond) += per-(sample, channel) sums of d pre (atomics).
 * mi_pcnn_small_mm: out[i][j] (+)= sum_k A[i*sai + k*sak] B[k*sbk + j*sbj] (conditioning biases and their weight gradient).
 * mi_pcnn_head_fwd: ELU(h) -> 1x1 to 256*Cc logits (w [256*Cc][Ch], class k of colour col is column k*Cc + col) -> log-sum-exp ->
 *   NLL at the reference's truncated target of img (NCHW, fp32) -> lse[N*HW*Cc], partial[mi_pcnn_head_partials], and
 *   *loss = mean bits per dim.  The logits are not written.
 * mi_pcnn_head_dlogits: dl[p][k*Cc + col] = (softmax - onehot) * (*gscale, nullable = 1) / (N*Cc*HW*ln 2), recomputed from lse.
 * mi_pcnn_sample_step: at pixel *counter (raster order over H*W) pick, for every (sample, colour), k = min{k : cdf_k > u} under the
 *   fp32 softmax of its 256 logits (clamped to 255; u = uniforms[pixel][n*Cc + col]) and write k/255 (2k/255 - 1 when normalize)
 *   into img (NCHW) and xin (NHWC, pixel pitch ldx) -- unless no sample has -1 at that pixel; then *counter += 1.  One workgroup.
 * mi_pcnn_zero: zero fill on the stream (a kernel node under graph capture). */
#define MI_PCNN_MAX_TAPS 25
#define MI_PCNN_EPI_PLAIN 0
#define MI_PCNN_EPI_GATE_TS 1
#define MI_PCNN_EPI_GATE_TT 2
#define MI_PCNN_EPI_ELU_GRAD 3
#define MI_PCNN_MODE_FP32 0
#define MI_PCNN_MODE_BF16 1
typedef struct MiPcnnConvDesc {
    int N, H, W;
    int Cin, ldx;             /* channels of the tapped source (contraction rows per tap) and its pixel pitch */
    int Cout, ldy;            /* GEMM columns and the pixel pitch of y (gated: of the gated output) */
    int ntaps;
    int tap_dy[MI_PCNN_MAX_TAPS], tap_dx[MI_PCNN_MAX_TAPS], tap_w[MI_PCNN_MAX_TAPS];
    int w_sk, w_sc;
    int C2, ldx2, w2_sk, w2_sc;
    int epi, elu_in, accumulate, gate_C;
    int ldpre, ldcond, ldr, ldaux;
    int mode;                 /* MI_PCNN_MODE_FP32: fp32-exact MFMA; MI_PCNN_MODE_BF16: bf16 operands, fp32 accumulate */
} MiPcnnConvDesc;
int mi_pcnn_conv_supported(const MiPcnnConvDesc* d);
int mi_pcnn_conv(const MiPcnnConvDesc* d, const float* x, const float* w, const float* bias, const float* x2, const float* w2,
                 const float* bias2, const float* cond, const float* res, const float* aux, float* y, float* pre, void* stream);
int mi_pcnn_wgrad_supported(const MiPcnnConvDesc* d);
int mi_pcnn_wgrad(const MiPcnnConvDesc* d, const float* x, const float* dy, int lddy, float* dw, void* stream);
int mi_pcnn_colsum(int M, int C, const float* g, int ld, float* out, float* out2, void* stream);
int mi_pcnn_gate_bwd_supported(int C);
int mi_pcnn_gate_bwd(int N, int HW, int C, int kind, const float* pre, int ldpre, const float* cond, int ldcond, const float* dout,
                     int ldo, float* dpre, int lddp, float* dcond, void* stream);
int mi_pcnn_small_mm(int I, int J, int Kd, const float* A, int sai, int sak, const float* B, int sbk, int sbj, float* out, int ldo,
                     int accumulate, void* stream);
/* conditioning from int64 labels (out-of-range labels contribute nothing): out[n][j] = w[j][labels[n]];
 * dw[j][labels[n]] += dcond[n][j] (atomics).  w: the cond_proj weights as one [J][ncls] matrix. */
int mi_pcnn_cond_rows(int N, int J, int ncls, const int64_t* labels, const float* w, float* out, int ldo, void* stream);
int mi_pcnn_cond_wgrad(int N, int J, int ncls, const int64_t* labels, const float* dcond, int ldd, float* dw, void* stream);
int mi_pcnn_head_supported(int Cc, int Ch);
int mi_pcnn_head_partials(int N, int HW, int Cc);
int mi_pcnn_head_fwd(int N, int Cc, int HW, int Ch, const float* h, int ldh, const float* w, const float* b, const float* img,
                     int normalize, float* lse, float* partial, float* loss, void* stream);
int mi_pcnn_head_dlogits(int N, int Cc, int HW, int Ch, const float* h, int ldh, const float* w, const float* b, const float* img,
                         int normalize, const float* lse, const float* gscale, float* dl, void* stream);
int mi_pcnn_sample_supported(int N, int Cc, int Ch);
int mi_pcnn_sample_step(int N, int Cc, int H, int W, int Ch, const float* h, int ldh, const float* w, const float* b, int* counter,
                        const float* uniforms, float* img, float* xin, int ldx, int normalize, void* stream);
int mi_pcnn_zero(void* p, size_t bytes, void* stream);

/* ---- MADE operators (reference src/models/made.py; csrc/made.hip) ----------------------------------------------------------------
 * A masked linear layer y = act(x (W .* M)^T + b) with W the PyTorch [out][in] weight read in place and the mask M given by two
 * int32 degree vectors: M[o][i] = deg_out[o] >= deg_in[i].  The kernels SELECT the live weights (a masked weight is never read
 * into a product; a non-finite input meets only live weights), run on fp32-exact MFMA (MI_MADE_MODE_FP32) or on bf16 operands
 * with fp32 accumulation (MI_MADE_MODE_BF16), and keep every stored value fp32.
 * mi_made_supported: D = C*H*W >= 1 pixels, C 1..4, hidden a multiple of 4 in 4..8192.
 * mi_made_linear: y[n][o] = act(sum over live i of x[n][i] W[o][i] + b[o]), act = sigmoid when act != 0.  No atomics: bit-reproducible.
 * mi_made_dgrad: dx[n][i] = (sum over live o of gy[n][o] W[o][i]) * s(1 - s), s = s_in[n][i] (nullable: no factor); split over o
 *   into `work` (mi_made_dgrad_workspace bytes), summed in a fixed order.
 * mi_made_wgrad: dW[o][i] = sum_n gy[n][o] x[n][i] written for the live entries only (masked entries are never written) and
 *   db[o] = sum_n gy[n][o] (written, not accumulated).
 * mi_made_head_fwd: the output head (hidden h [N][Hd] -> 256*D logits, unit d*256 + a = class a of pixel d) fused with the
 *   log-sum-exp and the NLL at the reference's truncated target of img ([N][D] fp32): lse[n][d], partial[mi_made_head_partials],
 *   *loss = mean bits per dim.  The logits are not written.
 * mi_made_head_dlogits: dl[n][d*256 + a] = (softmax - onehot) * (*gscale, nullable = 1) / (N*D*ln 2), recomputed from lse.
 *   Non-finite activations: unlike mi_made_linear and mi_made_head_rows, mi_made_head_fwd and mi_made_head_dlogits do NOT take a
 *   non-finite h out of the matrix-core operand.  A NaN or +-Inf in h[n][i] meets the 0 that stands for a masked weight (NaN * 0 and
 *   Inf * 0 are NaN), so every logit of row n becomes NaN, whatever the degrees: lse[n][:], the loss and dl[n][:] are NaN.  Training
 *   feeds them sigmoid outputs, which are finite for every finite input.
 * mi_made_head_rows: logits[n][c*256 + a] of the C units at position *pos of the H*W raster (pixel c*HW + *pos): the sampler's
 *   head, 256*C rows of the head only.
 * mi_made_sample_step: at position *counter, for every (sample, channel) k = min{k : cdf_k > u} under the fp32 softmax of its
 *   logits (clamped to 255; u = uniforms[pos][n*C + c]) written as k/255 (2k/255 - 1 when normalize) into img [N][C][HW] -- unless
 *   no sample and no channel holds -1 there; then *counter += 1.  One workgroup. */
#define MI_MADE_MODE_FP32 0
#define MI_MADE_MODE_BF16 1
int mi_made_supported(int D, int hidden, int C);
int mi_made_linear(int mode, int N, int in, int out, const float* x, int ldx, const float* w, const float* b, const int* deg_in,
                   const int* deg_out, int act, float* y, int ldy, void* stream);
size_t mi_made_dgrad_workspace(int N, int in, int out);
int mi_made_dgrad(int mode, int N, int in, int out, const float* gy, long long ldg, const float* w, const int* deg_in, const int* deg_out,
                  const float* s_in, int lds, float* work, float* dx, int lddx, void* stream);
int mi_made_wgrad(int mode, int N, int in, int out, const float* gy, long long ldg, const float* x, int ldx, const int* deg_in,
                  const int* deg_out, float* dw, float* db, void* stream);
int mi_made_head_partials(int N, int D);
int mi_made_head_fwd(int mode, int N, int D, int Hd, const float* h, int ldh, const float* w, const float* b, const int* deg_in,
                     const int* deg_out, const float* img, int normalize, float* lse, float* partial, float* loss, void* stream);
int mi_made_head_dlogits(int mode, int N, int D, int Hd, const float* h, int ldh, const float* w, const float* b, const int* deg_in,
                         const int* deg_out, const float* img, int normalize, const float* lse, const float* gscale, float* dl,
                         void* stream);
int mi_made_head_rows(int mode, int N, int C, int HW, int Hd, const float* h, int ldh, const float* w, const float* b, const int* deg_in,
                      const int* deg_out, const int* pos, float* logits, void* stream);
int mi_made_sample_step(int N, int C, int HW, const float* logits, int* counter, const float* uniforms, float* img, int normalize,
                        void* stream);

/* ---- BiGAN's pair head (reference src/models/BiGAN.py:100-126, all of D(x, z) but dis_x's conv trunk; csrc/pair_disc.hip) ----
 * 2 N rows as two segments (0: real pairs, 1: fake pairs), H = 128:
 *   dis_z    code [L] -> Linear(L,H) -> GroupNorm(1,H) -> LeakyReLU(0.2) -> Linear(H,H) -> BatchNorm1d(H) per segment -> LeakyReLU
 *            -> Linear(H,H) -> LeakyReLU = zf
 *   dis_pair cat(zf, xf) -> Linear(2H,H) -> GroupNorm(1,H) -> LeakyReLU -> Linear(H,1) = logit
 * e [N][lde >= L]: segment 0's code rows; z [N][ldz >= L]: segment 1's; xf [2N][ldf >= H]: dis_x's output rows.  All read in place.
 * params / grads: sixteen pointers, weights input-major ([in][out]): dis_z's w1 [L][H], b1, gamma1, beta1, w2 [H][H], b2, gamma2, beta2
 *   (BatchNorm1d's), w3 [H][H], b3; dis_pair's wp [2H][H], bp, gamma, beta, wc [H], bc [1].  The parameter pointers are 16-byte aligned.
 * supported: H == 128, 1 <= L <= 128, N >= 2 per segment in training mode (N >= 1 in evaluation mode), N <= MI_PAIR_DISC_NMAX.
 * fwd (3 launches): training: batch statistics per segment (biased variance), running_mean / running_var (nullable together) updated twice,
 *   segment 0 first (unbiased variance), *num_batches_tracked += 2; evaluation: both segments use the running statistics, nothing is
 *   updated.  loss_mode 0 vanilla, 1 lsgan, 2 hinge (mi_adv_loss' formulas).  Outputs, every element stored: logit [2N]; dlogit_g,
 *   dlogit_d [2N] = d g_loss / d logit and d d_loss / d logit (g_loss: segment 0 against False + segment 1 against True; d_loss: the
 *   opposite targets; each a sum of two per-segment means); out6 = g_loss, d_loss, mean logit of segment 0, of segment 1, d_loss' two
 *   terms; tape (mi_pair_disc_tape_floats).  workspace: mi_pair_disc_workspace_floats floats, any content; tape and workspace 16-byte aligned.
 * bwd, from the forward's inputs and tape, into a workspace of the same size (any content):
 *   dxf != NULL (input gradients, from dlogit_g; 2 launches, 1 without de): dxf [2N][lddxf >= H] and de [N][ldde >= L] (nullable; segment 0's
 *     code gradient) = (accumulate_in ? old : 0) + in_scale * gradient.  Segment 1's code gets no gradient.
 *   grads != NULL (parameter gradients, from dlogit_d; 3 launches): g = (accumulate_params ? g : 0) + param_scale * gradient for the sixteen;
 *     dxf_d [2N][H] dense (nullable) = d d_loss / d xf, stored.
 *   Both in one call: 3 launches, the same bits as two calls. */
#define MI_PAIR_DISC_NMAX (1 << 20)
int mi_pair_disc_supported(int N, int L, int H, int training);
size_t mi_pair_disc_tape_floats(int N, int H);
size_t mi_pair_disc_workspace_floats(int N, int H);
int mi_pair_disc_fwd(int N, int L, int H, const float* e, int lde, const float* z, int ldz, const float* xf, int ldf,
                     const float* const* params, int training, int loss_mode, float momentum, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float* tape, float* workspace, float* logit, float* dlogit_g, float* dlogit_d, float* out6,
                     void* stream);
int mi_pair_disc_bwd(int N, int L, int H, const float* e, int lde, const float* z, int ldz, const float* xf, int ldf,
                     const float* const* params, int training, const float* tape, float* workspace, const float* dlogit_g,
                     const float* dlogit_d, float* dxf, int lddxf, float* de, int ldde, float in_scale, int accumulate_in, float* const* grads,
                     float* dxf_d, float param_scale, int accumulate_params, void* stream);

#ifdef __cplusplus
}
#endif
#endif
