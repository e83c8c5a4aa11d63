// PixelCNN operators (reference src/models/pixelcnn.py): masked dilated convolutions as implicit GEMMs over the live taps only,
// the gated epilogues of GatedMaskedConv (tanh * sigmoid on the vertical stack, tanh * tanh on the horizontal one), the gate
// backward with the per-(sample, channel) sums of class conditioning, the output head (ELU -> 1x1 to 256 * C -> log-sum-exp -> NLL
// at the target, logits never written) and the sampling step (softmax at one pixel, inverse CDF on a uniform, device-side pixel
// counter).  All activations are fp32 NHWC; weights are read in PyTorch's [Cout][Cin][KH][KW] layout through two strides, so
// the forward and the data gradient are the same kernel with the weight's roles swapped and the tap offsets negated.
//
// One conv kernel (pcnn_conv_kernel): a 64-pixel x 64-column tile per workgroup, 256 threads with 4 x 4 fp32 accumulators each,
// the contraction over (live tap, input channel) [+ the channels of a second, 1x1 source] staged 16 deep through LDS.  In the
// gated epilogues the tile's 64 columns are 32 channel pairs (c, c + C), so every thread owns both halves of the channels it
// gates.  Matrix cores in both modes: fp32-exact v_mfma_f32_32x32x2_f32 (MI_PCNN_MODE_FP32) or bf16 operands rounded at the MFMA with
// fp32 accumulation (v_mfma_f32_32x32x16_bf16, MI_PCNN_MODE_BF16); each wave owns a 32 x 32 block, the epilogue reads it back via LDS.
#include "common.h"
#include "ar_sample.h"

namespace {

constexpr int PC_TM = 64, PC_TN = 64, PC_TK = 16;

__device__ __forceinline__ float elu_f(float v) { return v > 0.f ? v : expm1f(v); }
__device__ __forceinline__ float elu_d(float v) { return v > 0.f ? 1.f : expf(v); }
__device__ __forceinline__ float sigm_f(float v) { return 1.f / (1.f + expf(-v)); }

typedef float f32x16_t __attribute__((ext_vector_type(16)));

// C[64 x 64] += A^T B on one 16-deep LDS chunk (A: As[k][row], B: Bs[k][col]); wave w owns the 32 x 32 block (w / 2, w % 2).
// MODE 0: v_mfma_f32_32x32x2_f32 (fp32-exact products); MODE 1: both operands rounded to bf16, v_mfma_f32_32x32x16_bf16, fp32 accumulate.
template <int MODE>
__device__ __forceinline__ void pc_tile_mma(const float (*As)[PC_TM + 4], const float (*Bs)[PC_TN + 4], f32x16_t& acc, int rb, int cb, int lane) {
    const int r = lane & 31, h = lane >> 5;
    if constexpr (MODE == 0) {
#pragma unroll
        for (int s = 0; s < PC_TK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + h][rb + r], Bs[2 * s + h][cb + r], acc, 0, 0, 0);
    } else {
        bf16x8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] = (__bf16)As[h * 8 + e][rb + r]; b[e] = (__bf16)Bs[h * 8 + e][cb + r]; }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
}
// the wave's MFMA accumulators -> Cs[row][col] (32 x 32 output layout: register q is row 8 (q / 4) + 4 (lane / 32) + q % 4, column lane % 32)
__device__ __forceinline__ void pc_stash(float (*Cs)[PC_TN + 1], const f32x16_t& acc, int rb, int cb, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < 16; ++q) Cs[rb + 8 * (q >> 2) + 4 * h + (q & 3)][cb + r] = acc[q];
}

struct ConvArgs {
    MiPcnnConvDesc d;
    const float* x; const float* w; const float* bias;
    const float* x2; const float* w2; const float* bias2;
    const float* cond; const float* res; const float* aux;
    float* y; float* pre;
};

// column j of a tile -> output channel, or -1 past the end
__device__ __forceinline__ int pc_col(const MiPcnnConvDesc& d, int tile, int j) {
    if (d.epi == MI_PCNN_EPI_GATE_TS || d.epi == MI_PCNN_EPI_GATE_TT) {
        const int c = tile * 32 + (j & 31);
        return c < d.gate_C ? c + (j >> 5) * d.gate_C : -1;
    }
    const int c = tile * PC_TN + j;
    return c < d.Cout ? c : -1;
}

template <int MODE>
__global__ __launch_bounds__(256) void pcnn_conv_kernel(ConvArgs a) {
    const MiPcnnConvDesc& d = a.d;
    __shared__ float As[PC_TK][PC_TM + 4];
    __shared__ float Bs[PC_TK][PC_TN + 4];
    __shared__ float Cs[PC_TM][PC_TN + 1];
    const int lane = threadIdx.x & 63, rb = (threadIdx.x >> 7) * 32, cb = ((threadIdx.x >> 6) & 1) * 32;
    f32x16_t macc;
#pragma unroll
    for (int q = 0; q < 16; ++q) macc[q] = 0.f;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int HW = d.H * d.W, P = d.N * HW;
    const int m0 = blockIdx.x * PC_TM;
    const int K1 = d.ntaps * d.Cin, K = K1 + d.C2;
    // staging roles: the thread loads k-row (tid & 15) of pixels (tid >> 4) + 16 i, and of columns (tid >> 4) + 16 i
    const int kk = tid & 15;
    int pn[4], py[4], px[4], pcol[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = m0 + (tid >> 4) + 16 * i;
        if (p < P) { pn[i] = p / HW; const int r = p - pn[i] * HW; py[i] = r / d.W; px[i] = r - py[i] * d.W; }
        else { pn[i] = -1; py[i] = px[i] = 0; }
        pcol[i] = pc_col(d, blockIdx.y, (tid >> 4) + 16 * i);
    }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int k0 = 0; k0 < K; k0 += PC_TK) {
        const int k = k0 + kk;
        int t = 0, c = 0;
        if (k < K1) { t = k / d.Cin; c = k - t * d.Cin; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = 0.f, wv = 0.f;
            if (k < K1) {
                if (pn[i] >= 0) {
                    const int yy = py[i] + d.tap_dy[t], xx = px[i] + d.tap_dx[t];
                    if (yy >= 0 && yy < d.H && xx >= 0 && xx < d.W) {
                        v = a.x[((size_t)pn[i] * HW + (size_t)yy * d.W + xx) * d.ldx + c];
                        if (d.elu_in) v = elu_f(v);
                    }
                }
                if (pcol[i] >= 0) wv = a.w[(size_t)c * d.w_sk + (size_t)pcol[i] * d.w_sc + d.tap_w[t]];
            } else if (k < K) {
                const int c2 = k - K1;
                if (pn[i] >= 0) v = a.x2[(size_t)(m0 + (tid >> 4) + 16 * i) * d.ldx2 + c2];
                if (pcol[i] >= 0) wv = a.w2[(size_t)c2 * d.w2_sk + (size_t)pcol[i] * d.w2_sc];
            }
            As[kk][(tid >> 4) + 16 * i] = v;
            Bs[kk][(tid >> 4) + 16 * i] = wv;
        }
        __syncthreads();
        pc_tile_mma<MODE>(As, Bs, macc, rb, cb, lane);
        __syncthreads();
    }
    pc_stash(Cs, macc, rb, cb, lane);
    __syncthreads();
    {
        const int cc[4] = {tx * 2, tx * 2 + 1, 32 + tx * 2, 32 + tx * 2 + 1};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = Cs[ty * 4 + i][cc[j]];
    }

    const int cols[4] = {tx * 2, tx * 2 + 1, 32 + tx * 2, 32 + tx * 2 + 1};
    int ch[4];
    float bsum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ch[j] = pc_col(d, blockIdx.y, cols[j]);
        bsum[j] = 0.f;
        if (ch[j] >= 0) {
            if (a.bias) bsum[j] += a.bias[ch[j]];
            if (a.bias2) bsum[j] += a.bias2[ch[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = m0 + ty * 4 + i;
        if (p >= P) continue;
        const int n = p / HW;
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = acc[i][j] + bsum[j];
        if (d.epi == MI_PCNN_EPI_GATE_TS || d.epi == MI_PCNN_EPI_GATE_TT) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {                         // pair (cols[j], cols[j + 2]) = channels (c, c + C)
                if (ch[j] < 0) continue;
                const int c = ch[j];
                a.pre[(size_t)p * d.ldpre + c] = r[j];
                a.pre[(size_t)p * d.ldpre + c + d.gate_C] = r[j + 2];
                float lo = r[j], hi = r[j + 2];
                if (a.cond) { lo += a.cond[(size_t)n * d.ldcond + c]; hi += a.cond[(size_t)n * d.ldcond + c + d.gate_C]; }
                const float g = d.epi == MI_PCNN_EPI_GATE_TS ? sigm_f(hi) : tanhf(hi);
                a.y[(size_t)p * d.ldy + c] = tanhf(lo) * g;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (ch[j] < 0) continue;
                float v = r[j];
                float* yp = a.y + (size_t)p * d.ldy + ch[j];
                if (a.res) v += a.res[(size_t)p * d.ldr + ch[j]];
                if (d.epi == MI_PCNN_EPI_ELU_GRAD) v *= elu_d(a.aux[(size_t)p * d.ldaux + ch[j]]);
                if (d.accumulate) v += *yp;
                *yp = v;
            }
        }
    }
}

// dW[row c][col o][tap] += sum_p x[p + off_t][c] * dy[p][o]  (x optionally through ELU).  Grid: (row tiles, col tiles, taps * splits);
// every workgroup adds its pixel range's 64 x 64 block with atomics.
template <int MODE>
__global__ __launch_bounds__(256) void pcnn_wgrad_kernel(MiPcnnConvDesc d, const float* __restrict__ x, const float* __restrict__ dy,
                                                         int lddy, float* __restrict__ dw, int splits, int span) {
    __shared__ float As[PC_TK][PC_TM + 4];
    __shared__ float Bs[PC_TK][PC_TN + 4];
    __shared__ float Cs[PC_TM][PC_TN + 1];
    const int lane = threadIdx.x & 63, rb = (threadIdx.x >> 7) * 32, cb = ((threadIdx.x >> 6) & 1) * 32;
    f32x16_t macc;
#pragma unroll
    for (int q = 0; q < 16; ++q) macc[q] = 0.f;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int HW = d.H * d.W, P = d.N * HW;
    const int t = blockIdx.z / splits, s = blockIdx.z - t * splits;
    const int p0 = s * span, p1 = min(P, p0 + span);
    const int c0 = blockIdx.x * PC_TM, o0 = blockIdx.y * PC_TN;
    const int lc = tid & 63, lp = tid >> 6;                     // staging: column lc of pixels lp + 4 i
    const int dyo = d.tap_dy[t], dxo = d.tap_dx[t];
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int q0 = p0; q0 < p1; q0 += PC_TK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pl = lp + 4 * i, p = q0 + pl;
            float v = 0.f, g = 0.f;
            if (p < p1) {
                if (c0 + lc < d.Cin) {
                    const int n = p / HW, r = p - n * HW, yy = r / d.W + dyo, xx = r % d.W + dxo;
                    if (yy >= 0 && yy < d.H && xx >= 0 && xx < d.W) {
                        v = x[((size_t)n * HW + (size_t)yy * d.W + xx) * d.ldx + c0 + lc];
                        if (d.elu_in) v = elu_f(v);
                    }
                }
                if (o0 + lc < d.Cout) g = dy[(size_t)p * lddy + o0 + lc];
            }
            As[pl][lc] = v;
            Bs[pl][lc] = g;
        }
        __syncthreads();
        pc_tile_mma<MODE>(As, Bs, macc, rb, cb, lane);
        __syncthreads();
    }
    pc_stash(Cs, macc, rb, cb, lane);
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = Cs[ty * 4 + i][tx * 4 + j];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty * 4 + i;
        if (c >= d.Cin) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = o0 + tx * 4 + j;
            if (o < d.Cout) atomicAdd(dw + (size_t)c * d.w_sk + (size_t)o * d.w_sc + d.tap_w[t], acc[i][j]);
        }
    }
}

// out[o] (and out2[o]) += sum_p g[p][o]; grid (col tiles of 64, row splits)
__global__ __launch_bounds__(256) void pcnn_colsum_kernel(int M, int C, const float* __restrict__ g, int ld, float* out, float* out2, int span) {
    __shared__ float red[4][64];
    const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6, c = blockIdx.x * 64 + lc;
    const int r0 = blockIdx.y * span, r1 = min(M, r0 + span);
    float s = 0.f;
    if (c < C)
        for (int r = r0 + lr; r < r1; r += 4) s += g[(size_t)r * ld + c];
    red[lr][lc] = s;
    __syncthreads();
    if (lr == 0 && c < C) {
        s = red[0][lc] + red[1][lc] + red[2][lc] + red[3][lc];
        if (out) atomicAdd(out + c, s);
        if (out2) atomicAdd(out2 + c, s);
    }
}

// d pre of a gate from the saved raw pre-activations (+ conditioning bias) and d out; dcond[n][ch] += sum over the sample's pixels
template <bool TS>
__global__ __launch_bounds__(256) void pcnn_gate_bwd_kernel(int HW, int C, const float* __restrict__ pre, int ldpre,
                                                            const float* __restrict__ cond, int ldcond, const float* __restrict__ dout,
                                                            int ldo, float* __restrict__ dpre, int lddp, float* __restrict__ dcond, int pix_per_block) {
    extern __shared__ float red[];                              // [2C] when conditioned
    const int n = blockIdx.y;
    const int q0 = blockIdx.x * pix_per_block, q1 = min(HW, q0 + pix_per_block);
    if (dcond) {
        for (int i = threadIdx.x; i < 2 * C; i += 256) red[i] = 0.f;
        __syncthreads();
    }
    const int total = (q1 - q0) * C;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int pl = e / C, c = e - pl * C;
        const size_t p = (size_t)n * HW + q0 + pl;
        float lo = pre[p * ldpre + c], hi = pre[p * ldpre + C + c];
        if (cond) { lo += cond[(size_t)n * ldcond + c]; hi += cond[(size_t)n * ldcond + C + c]; }
        const float g = dout[p * ldo + c];
        const float ta = tanhf(lo);
        float da, db;
        if (TS) { const float sg = sigm_f(hi); da = g * sg * (1.f - ta * ta); db = g * ta * sg * (1.f - sg); }
        else { const float tb = tanhf(hi); da = g * tb * (1.f - ta * ta); db = g * ta * (1.f - tb * tb); }
        dpre[p * lddp + c] = da;
        dpre[p * lddp + C + c] = db;
        if (dcond) { atomicAdd(&red[c], da); atomicAdd(&red[C + c], db); }
    }
    if (dcond) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * C; i += 256) atomicAdd(dcond + (size_t)n * ldcond + i, red[i]);
    }
}

// out[i][j] (+)= sum_k A[i sai + k sak] B[k sbk + j sbj]: the class-conditioning biases (one-hot x cond_proj weights) and their gradient
__global__ void pcnn_small_mm_kernel(int I, int J, int Kd, const float* __restrict__ A, int sai, int sak, const float* __restrict__ B,
                                     int sbk, int sbj, float* __restrict__ out, int ldo, int accumulate) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= I * J) return;
    const int i = idx / J, j = idx - i * J;
    float s = 0.f;
    for (int k = 0; k < Kd; ++k) s = fmaf(A[(size_t)i * sai + (size_t)k * sak], B[(size_t)k * sbk + (size_t)j * sbj], s);
    float* o = out + (size_t)i * ldo + j;
    *o = accumulate ? *o + s : s;
}

// class conditioning from integer labels: rows[n][j] = W[j][label[n]] (forward), dW[j][label[n]] += dcond[n][j] (backward)
__global__ void pcnn_cond_rows_kernel(int N, int J, int ncls, const int64_t* __restrict__ labels, const float* __restrict__ w,
                                      float* __restrict__ out, int ldo) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * J) return;
    const int n = idx / J, j = idx - n * J;
    const int64_t l = labels[n];
    out[(size_t)n * ldo + j] = (l >= 0 && l < ncls) ? w[(size_t)j * ncls + l] : 0.f;
}
__global__ void pcnn_cond_wgrad_kernel(int N, int J, int ncls, const int64_t* __restrict__ labels, const float* __restrict__ dcond, int ldd,
                                       float* __restrict__ dw) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * J) return;
    const int n = idx / J, j = idx - n * J;
    const int64_t l = labels[n];
    if (l >= 0 && l < ncls) atomicAdd(dw + (size_t)j * ncls + l, dcond[(size_t)n * ldd + j]);
}

// The reference's target: (x * 255).long() or ((x + 1) / 2 * 255).long(), fp32 then truncation toward zero (clamped to the classes)
__device__ __forceinline__ int pcnn_target(float xv, int normalize) {
    float v;
    if (normalize) { const float a = __fadd_rn(xv, 1.f); v = __fmul_rn(__fdiv_rn(a, 2.f), 255.f); }
    else v = __fmul_rn(xv, 255.f);
    int t = (int)v;
    return t < 0 ? 0 : (t > 255 ? 255 : t);
}

// Output head.  Unit u = (pixel p, colour col), four lanes per unit, 64 classes per lane; logit(k) = b[o] + sum_c elu(h[p][c]) W[o][c],
// o = k * Cc + col.  Forward: online log-sum-exp, NLL at the target, lse[u] saved, one partial sum per workgroup.
// Backward (dl non-null): dl[p][o] = (softmax - onehot) * scale * (*gscale), lse from the forward.
constexpr int HEAD_UNITS = 64;
__global__ __launch_bounds__(256) void pcnn_head_kernel(int N, int Cc, int HW, int Ch, const float* __restrict__ h, int ldh,
                                                        const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ img,
                                                        int normalize, float* __restrict__ lse, float* __restrict__ partial,
                                                        float* __restrict__ dl, float scale, const float* __restrict__ gscale) {
    extern __shared__ float ha[];                                // [HEAD_UNITS][Ch + 1]: ELU'd hidden rows of the block's units
    __shared__ float red[4];
    const int U = N * HW * Cc, u0 = blockIdx.x * HEAD_UNITS;
    const int ld = Ch + 1;
    for (int e = threadIdx.x; e < HEAD_UNITS * Ch; e += 256) {
        const int ul = e / Ch, c = e - ul * Ch, u = u0 + ul;
        ha[ul * ld + c] = u < U ? elu_f(h[(size_t)(u / Cc) * ldh + c]) : 0.f;
    }
    __syncthreads();
    const int ul = threadIdx.x >> 2, q = threadIdx.x & 3, u = u0 + ul;
    float nll = 0.f;
    if (u < U) {
        const int p = u / Cc, col = u - p * Cc, n = p / HW, hw = p - n * HW;
        const int tgt = pcnn_target(img[((size_t)n * Cc + col) * HW + hw], normalize);
        const float* a = ha + ul * ld;
        if (!dl) {
            float m = -INFINITY, s = 0.f, lt = 0.f;
            for (int j = 0; j < 64; ++j) {
                const int k = q * 64 + j, o = k * Cc + col;
                const float* wr = w + (size_t)o * Ch;
                float l = b[o];
                for (int c = 0; c < Ch; ++c) l = fmaf(a[c], wr[c], l);
                if (k == tgt) lt = l;
                if (l > m) { s = s * expf(m - l) + 1.f; m = l; } else s += expf(l - m);
            }
#pragma unroll
            for (int off = 1; off < 4; off <<= 1) {
                const float m2 = __shfl_xor(m, off, 4), s2 = __shfl_xor(s, off, 4), lt2 = __shfl_xor(lt, off, 4);
                const float mm = fmaxf(m, m2);
                s = s * expf(m - mm) + s2 * expf(m2 - mm);
                m = mm;
                lt += lt2;                                     // only the lane that owns the target class holds a non-zero
            }
            const float L = m + logf(s);
            if (q == 0) { lse[u] = L; nll = L - lt; }
        } else {
            const float L = lse[u], g = scale * (gscale ? *gscale : 1.f);
            for (int j = 0; j < 64; ++j) {
                const int k = q * 64 + j, o = k * Cc + col;
                const float* wr = w + (size_t)o * Ch;
                float l = b[o];
                for (int c = 0; c < Ch; ++c) l = fmaf(a[c], wr[c], l);
                dl[(size_t)p * (256 * Cc) + o] = (expf(l - L) - (k == tgt ? 1.f : 0.f)) * g;
            }
        }
    }
    if (dl) return;
    for (int off = 32; off > 0; off >>= 1) nll += __shfl_xor(nll, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nll;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void pcnn_reduce_kernel(int n, const float* __restrict__ partial, float scale, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1] + red[2] + red[3]) * scale;
}

// One sampling step at pixel *counter (raster order), one workgroup of 16 waves, a wave per (sample, colour) unit at a time.
// The reference skips the pixel only when no sample has -1 there; otherwise the value is written for the whole batch.
__global__ __launch_bounds__(1024) void pcnn_sample_kernel(int N, int Cc, int H, int W, int Ch, const float* __restrict__ h, int ldh,
                                                           const float* __restrict__ w, const float* __restrict__ b, int* counter,
                                                           const float* __restrict__ uni, float* img, float* xin, int ldx, int normalize) {
    __shared__ int any_missing;
    const int HW = H * W, pix = *counter;
    if (threadIdx.x == 0) any_missing = 0;
    __syncthreads();
    if (pix < HW) {
        for (int i = threadIdx.x; i < N * Cc; i += blockDim.x)
            if (img[(size_t)i * HW + pix] == -1.f) any_missing = 1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (pix < HW && any_missing) {
        for (int u = wave; u < N * Cc; u += nw) {
            const int n = u / Cc, col = u - n * Cc;
            const float* hr = h + ((size_t)n * HW + pix) * ldh;
            float l[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = (lane * 4 + j) * Cc + col;
                const float* wr = w + (size_t)o * Ch;
                float s = b[o];
                for (int c = 0; c < Ch; ++c) s = fmaf(elu_f(hr[c]), wr[c], s);
                l[j] = s;
            }
            const int k = ar_inverse_cdf_pick(l, uni[(size_t)pix * N * Cc + u], lane);
            if (lane == 0) {
                float v = (float)k / 255.f;
                if (normalize) v = v * 2.f - 1.f;
                img[((size_t)n * Cc + col) * HW + pix] = v;
                xin[((size_t)n * HW + pix) * ldx + col] = v;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) counter[0] = pix + 1;
}

int pcnn_check_desc(const MiPcnnConvDesc* d) {
    if (!d) return 0;
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->Cin < 0 || d->Cout < 1 || d->ntaps < 0 || d->ntaps > MI_PCNN_MAX_TAPS) return 0;
    if ((size_t)d->N * d->H * d->W >= (1u << 31) / 64) return 0;
    if (d->ntaps * d->Cin + d->C2 < 1) return 0;
    if (d->epi < 0 || d->epi > MI_PCNN_EPI_ELU_GRAD) return 0;
    if (d->mode != MI_PCNN_MODE_FP32 && d->mode != MI_PCNN_MODE_BF16) return 0;
    if ((d->epi == MI_PCNN_EPI_GATE_TS || d->epi == MI_PCNN_EPI_GATE_TT) && (d->gate_C < 1 || d->Cout != 2 * d->gate_C)) return 0;
    return 1;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_pcnn_conv_supported(const MiPcnnConvDesc* d) { return pcnn_check_desc(d); }

extern "C" int mi_pcnn_conv(const MiPcnnConvDesc* d, const float* x, const float* w, const float* bias, const float* x2, const float* w2,
                            const float* bias2, const float* cond, const float* res, const float* aux, float* y, float* pre, void* stream) {
    MI_REQUIRE(pcnn_check_desc(d), "unsupported descriptor (mi_pcnn_conv_supported)");
    MI_REQUIRE(y && (d->ntaps * d->Cin == 0 || (x && w)) && (d->C2 == 0 || (x2 && w2)), "null operand");
    const bool gated = d->epi == MI_PCNN_EPI_GATE_TS || d->epi == MI_PCNN_EPI_GATE_TT;
    MI_REQUIRE(!gated || pre, "a gated epilogue needs pre");
    MI_REQUIRE(d->epi != MI_PCNN_EPI_ELU_GRAD || aux, "the ELU-gradient epilogue needs aux");
    ConvArgs a{*d, x, w, bias, x2, w2, bias2, cond, res, aux, y, pre};
    const int P = d->N * d->H * d->W;
    const int cols = gated ? (d->gate_C + 31) / 32 : (d->Cout + PC_TN - 1) / PC_TN;
    const dim3 grid((P + PC_TM - 1) / PC_TM, cols);
    if (d->mode == MI_PCNN_MODE_BF16) hipLaunchKernelGGL(pcnn_conv_kernel<1>, grid, dim3(256), 0, ST, a);
    else hipLaunchKernelGGL(pcnn_conv_kernel<0>, grid, dim3(256), 0, ST, a);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_wgrad_supported(const MiPcnnConvDesc* d) { return pcnn_check_desc(d) && d->ntaps >= 1 && d->Cin >= 1; }

extern "C" int mi_pcnn_wgrad(const MiPcnnConvDesc* d, const float* x, const float* dy, int lddy, float* dw, void* stream) {
    MI_REQUIRE(mi_pcnn_wgrad_supported(d), "unsupported descriptor (mi_pcnn_wgrad_supported)");
    MI_REQUIRE(x && dy && dw && lddy >= d->Cout, "null operand or lddy < Cout");
    const int P = d->N * d->H * d->W;
    const int span = 2048, splits = (P + span - 1) / span;
    const dim3 grid((d->Cin + PC_TM - 1) / PC_TM, (d->Cout + PC_TN - 1) / PC_TN, d->ntaps * splits);
    if (d->mode == MI_PCNN_MODE_BF16) hipLaunchKernelGGL(pcnn_wgrad_kernel<1>, grid, dim3(256), 0, ST, *d, x, dy, lddy, dw, splits, span);
    else hipLaunchKernelGGL(pcnn_wgrad_kernel<0>, grid, dim3(256), 0, ST, *d, x, dy, lddy, dw, splits, span);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_colsum(int M, int C, const float* g, int ld, float* out, float* out2, void* stream) {
    MI_REQUIRE(M >= 1 && C >= 1 && ld >= C && g && (out || out2), "bad arguments");
    const int span = 1024;
    hipLaunchKernelGGL(pcnn_colsum_kernel, dim3((C + 63) / 64, (M + span - 1) / span), dim3(256), 0, ST, M, C, g, ld, out, out2, span);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_gate_bwd_supported(int C) { return C >= 1 && C <= 4096; }

extern "C" int mi_pcnn_gate_bwd(int N, int HW, int C, int kind, const float* pre, int ldpre, const float* cond, int ldcond, const float* dout,
                                int ldo, float* dpre, int lddp, float* dcond, void* stream) {
    MI_REQUIRE(mi_pcnn_gate_bwd_supported(C) && N >= 1 && HW >= 1, "unsupported shape (mi_pcnn_gate_bwd_supported)");
    MI_REQUIRE(kind == MI_PCNN_EPI_GATE_TS || kind == MI_PCNN_EPI_GATE_TT, "kind: MI_PCNN_EPI_GATE_TS or MI_PCNN_EPI_GATE_TT");
    MI_REQUIRE(pre && dout && dpre && ldpre >= 2 * C && lddp >= 2 * C && ldo >= C, "null operand or short pitch");
    MI_REQUIRE(!dcond || ldcond >= 2 * C, "dcond needs ldcond >= 2C");
    const int ppb = max(1, min(HW, 8192 / C));
    const dim3 grid((HW + ppb - 1) / ppb, N);
    const size_t sh = dcond ? 2 * C * sizeof(float) : 0;
    if (kind == MI_PCNN_EPI_GATE_TS)
        hipLaunchKernelGGL(pcnn_gate_bwd_kernel<true>, grid, dim3(256), sh, ST, HW, C, pre, ldpre, cond, ldcond, dout, ldo, dpre, lddp, dcond, ppb);
    else
        hipLaunchKernelGGL(pcnn_gate_bwd_kernel<false>, grid, dim3(256), sh, ST, HW, C, pre, ldpre, cond, ldcond, dout, ldo, dpre, lddp, dcond, ppb);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_small_mm(int I, int J, int Kd, const float* A, int sai, int sak, const float* B, int sbk, int sbj, float* out, int ldo,
                                int accumulate, void* stream) {
    MI_REQUIRE(I >= 1 && J >= 1 && Kd >= 1 && A && B && out && ldo >= J, "bad arguments");
    const int n = I * J;
    hipLaunchKernelGGL(pcnn_small_mm_kernel, dim3((n + 255) / 256), dim3(256), 0, ST, I, J, Kd, A, sai, sak, B, sbk, sbj, out, ldo, accumulate);
    MI_LAUNCH_CHECK();
    return 0;
}

// the head stages HEAD_UNITS ELU'd rows of Ch + 1 floats in dynamic LDS: Ch <= 254 keeps it inside the default 64 KB
extern "C" int mi_pcnn_cond_rows(int N, int J, int ncls, const int64_t* labels, const float* w, float* out, int ldo, void* stream) {
    MI_REQUIRE(N >= 1 && J >= 1 && ncls >= 1 && labels && w && out && ldo >= J, "bad arguments");
    hipLaunchKernelGGL(pcnn_cond_rows_kernel, dim3((N * J + 255) / 256), dim3(256), 0, ST, N, J, ncls, labels, w, out, ldo);
    MI_LAUNCH_CHECK();
    return 0;
}
extern "C" int mi_pcnn_cond_wgrad(int N, int J, int ncls, const int64_t* labels, const float* dcond, int ldd, float* dw, void* stream) {
    MI_REQUIRE(N >= 1 && J >= 1 && ncls >= 1 && labels && dcond && dw && ldd >= J, "bad arguments");
    hipLaunchKernelGGL(pcnn_cond_wgrad_kernel, dim3((N * J + 255) / 256), dim3(256), 0, ST, N, J, ncls, labels, dcond, ldd, dw);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_head_supported(int Cc, int Ch) { return Cc >= 1 && Cc <= 4 && Ch >= 1 && (size_t)HEAD_UNITS * (Ch + 1) * 4 + 16 <= 65536; }
extern "C" int mi_pcnn_head_partials(int N, int HW, int Cc) { return (N * HW * Cc + HEAD_UNITS - 1) / HEAD_UNITS; }

extern "C" int mi_pcnn_head_fwd(int N, int Cc, int HW, int Ch, const float* h, int ldh, const float* w, const float* b, const float* img,
                                int normalize, float* lse, float* partial, float* loss, void* stream) {
    MI_REQUIRE(mi_pcnn_head_supported(Cc, Ch) && N >= 1 && HW >= 1, "unsupported shape (mi_pcnn_head_supported)");
    MI_REQUIRE(h && w && b && img && lse && partial && loss && ldh >= Ch, "null operand or short pitch");
    const int blocks = mi_pcnn_head_partials(N, HW, Cc);
    const size_t sh = (size_t)HEAD_UNITS * (Ch + 1) * sizeof(float);
    hipLaunchKernelGGL(pcnn_head_kernel, dim3(blocks), dim3(256), sh, ST, N, Cc, HW, Ch, h, ldh, w, b, img, normalize, lse, partial,
                       (float*)nullptr, 0.f, (const float*)nullptr);
    MI_LAUNCH_CHECK();
    const float ln2 = 0.693147182464599609375f;                 // torch.log(torch.tensor(2.)) in fp32: the reference's `log2` buffer
    hipLaunchKernelGGL(pcnn_reduce_kernel, dim3(1), dim3(256), 0, ST, blocks, (const float*)partial, 1.f / ((float)N * Cc * HW * ln2), loss);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_head_dlogits(int N, int Cc, int HW, int Ch, const float* h, int ldh, const float* w, const float* b, const float* img,
                                    int normalize, const float* lse, const float* gscale, float* dl, void* stream) {
    MI_REQUIRE(mi_pcnn_head_supported(Cc, Ch) && N >= 1 && HW >= 1, "unsupported shape (mi_pcnn_head_supported)");
    MI_REQUIRE(h && w && b && img && lse && dl && ldh >= Ch, "null operand or short pitch");
    const int blocks = mi_pcnn_head_partials(N, HW, Cc);
    const size_t sh = (size_t)HEAD_UNITS * (Ch + 1) * sizeof(float);
    const float ln2 = 0.693147182464599609375f;
    hipLaunchKernelGGL(pcnn_head_kernel, dim3(blocks), dim3(256), sh, ST, N, Cc, HW, Ch, h, ldh, w, b, img, normalize, (float*)lse,
                       (float*)nullptr, dl, 1.f / ((float)N * Cc * HW * ln2), gscale);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_sample_supported(int N, int Cc, int Ch) { return N >= 1 && Cc >= 1 && Cc <= 4 && Ch >= 1 && Ch <= 4096; }

extern "C" int mi_pcnn_sample_step(int N, int Cc, int H, int W, int Ch, const float* h, int ldh, const float* w, const float* b, int* counter,
                                   const float* uniforms, float* img, float* xin, int ldx, int normalize, void* stream) {
    MI_REQUIRE(mi_pcnn_sample_supported(N, Cc, Ch) && H >= 1 && W >= 1, "unsupported shape (mi_pcnn_sample_supported)");
    MI_REQUIRE(h && w && b && counter && uniforms && img && xin && ldh >= Ch && ldx >= Cc, "null operand or short pitch");
    hipLaunchKernelGGL(pcnn_sample_kernel, dim3(1), dim3(1024), 0, ST, N, Cc, H, W, Ch, h, ldh, w, b, counter, uniforms, img, xin, ldx, normalize);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pcnn_zero(void* p, size_t bytes, void* stream) {
    MI_REQUIRE(p && bytes % 4 == 0, "4-byte multiple");
    const hipError_t e = mi_zero_async(p, bytes, ST);
    if (e != hipSuccess) return mi_set_error((int)e, "mi_pcnn_zero: %s", hipGetErrorString(e));
    return 0;
}
