// MADE operators (reference src/models/made.py): masked linear layers, the fused output head and the sampling step.
//
// One GEMM core (made_gemm_kernel) serves every product.  C[m][c] = sum_k A[m][k] B[k][c], A[m][k] = a[m*sam + k*sak],
// B[k][c] = b[c*sbc + k*sbk].  Each wave owns RM x RN blocks of 32 x 32 (rows x columns) and streams its operands straight from
// global memory into registers, 16 contraction steps at a time, with no LDS: in step s of a chunk the lane (r, h) = (lane % 32,
// lane / 32) supplies k = 8h + s, so a lane's 8 values of a row (or column) are contiguous in k.  fp32 mode issues 8
// v_mfma_f32_32x32x2_f32 per chunk, bf16 mode rounds the same 8 values to bf16 and issues one v_mfma_f32_32x32x16_bf16.
//
// The mask is never read.  The weight operand is SELECTED where the degrees allow it (sel 1: deg_c[o] >= deg_k[i], the forward;
// sel 2: deg_k[o] >= deg_c[i], the data gradient) and is 0 elsewhere, so a masked weight never reaches the product.  A masked
// INPUT still meets that 0 in the matrix core, and NaN * 0 is NaN; the forward therefore takes non-finite activations out of the
// MFMA operand (as 0) and adds their products back, one by one, for the live weights only (a rare path, taken per wave and chunk
// only when a non-finite value is present).  The forward has no atomics and a fixed reduction order: it is bit-reproducible.
#include "common.h"
#include "ar_sample.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));

enum { EPI_Y = 0, EPI_WG = 1, EPI_LSE = 2, EPI_DL = 3 };

struct GemmArgs {
    int M, Nc, K;                        // rows, columns, contraction length
    const float* a; long long sam, sak;
    const float* b; long long sbc, sbk;
    const int* dk; const int* dc; int sel;
    int kspan;                           // contraction range of split blockIdx.z: [z kspan, (z + 1) kspan)
    int fix;                             // forward: exact handling of non-finite A values (see the file comment)
    const float* bias; int act;          // EPI_Y: + bias[o], then sigmoid when act
    float* y; long long ldy, zstride;    // EPI_Y / EPI_WG / EPI_DL output
    const int* dr;                       // EPI_WG: row degrees (written only where dr[row] >= dc[col])
    const float* img; int D, normalize;  // head: the image, D = C*H*W pixels
    float* lse; float* partial; const float* gscale; float scale;
    const int* pos; int remap_hw;        // sampler: column c -> head row ((c / 256) * remap_hw + *pos) * 256 + c % 256
};

__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ bool finite_f(float v) { return __builtin_isfinite(v); }

// The reference's target: (x * 255).long() or ((x + 1) / 2 * 255).long(): fp32, then truncation toward zero (clamped to the classes)
__device__ __forceinline__ int made_target(float xv, int normalize) {
    float v;
    if (normalize) { const float a = __fadd_rn(xv, 1.f); v = __fmul_rn(__fdiv_rn(a, 2.f), 255.f); }
    else v = __fmul_rn(xv, 255.f);
    int t = (int)v;
    return t < 0 ? 0 : (t > 255 ? 255 : t);
}

__device__ __forceinline__ long long col_to_o(const GemmArgs& g, int c, int p) {
    return g.remap_hw ? ((long long)(c >> 8) * g.remap_hw + p) * 256 + (c & 255) : (long long)c;
}

// 8 consecutive-k values of one row (ok = row in range) starting at k = kb; kc: the k stride is 1 (two 16-byte loads when aligned)
template <bool KC>
__device__ __forceinline__ void load8(const float* p, long long sk, int kleft, bool ok, float (&v)[8]) {
    if (KC && ok && kleft >= 8 && ((uintptr_t)p & 15) == 0) {
        const float4 x0 = reinterpret_cast<const float4*>(p)[0], x1 = reinterpret_cast<const float4*>(p)[1];
        v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (ok && e < kleft) ? p[KC ? e : e * sk] : 0.f;
}

template <int MODE, int RM, int RN, int WAVES, int EPI, bool AKC, bool BKC>
__global__ __launch_bounds__(WAVES * 64) void made_gemm_kernel(GemmArgs g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.y * (RM * 32);
    const int cw = blockIdx.x * (WAVES * RN * 32) + wave * (RN * 32);       // the wave's first column
    const int kbeg = blockIdx.z * g.kspan, kend = min(g.K, kbeg + g.kspan);
    const int p = g.remap_hw ? *g.pos : 0;
    constexpr bool FIXABLE = EPI == EPI_Y && BKC;                           // the forward products (the data gradient has BKC false)

    f32x16_t acc[RM][RN];
#pragma unroll
    for (int j = 0; j < RM; ++j)
#pragma unroll
        for (int jn = 0; jn < RN; ++jn)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][jn][q] = 0.f;

    long long ocol[RN];
    int dcol[RN];
    bool cok[RN];
#pragma unroll
    for (int jn = 0; jn < RN; ++jn) {
        const int c = cw + 32 * jn + r;
        cok[jn] = c < g.Nc;
        ocol[jn] = cok[jn] ? col_to_o(g, c, p) : 0;
        dcol[jn] = (cok[jn] && g.sel) ? g.dc[ocol[jn]] : 0;
    }

    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        const int kb = k0 + 8 * h, kleft = kend - kb;
        float av[RM][8], bv[RN][8];
#pragma unroll
        for (int j = 0; j < RM; ++j) {
            const int m = r0 + 32 * j + r;
            load8<AKC>(g.a + (long long)(m < g.M ? m : 0) * g.sam + (long long)kb * g.sak, g.sak, kleft, m < g.M, av[j]);
        }
        int dkv[8];
        if (g.sel) {
#pragma unroll
            for (int e = 0; e < 8; ++e) dkv[e] = e < kleft ? g.dk[kb + e] : 0;
        }
#pragma unroll
        for (int jn = 0; jn < RN; ++jn) {
            load8<BKC>(g.b + ocol[jn] * g.sbc + (long long)kb * g.sbk, g.sbk, kleft, cok[jn], bv[jn]);
            if (g.sel) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool live = g.sel == 1 ? dcol[jn] >= dkv[e] : dkv[e] >= dcol[jn];
                    bv[jn][e] = live ? bv[jn][e] : 0.f;
                }
            }
        }
        if (FIXABLE && g.fix) {
            bool bad = false;
#pragma unroll
            for (int j = 0; j < RM; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) bad |= !finite_f(av[j][e]);
            if (__any(bad)) {
#pragma unroll
                for (int j = 0; j < RM; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) av[j][e] = finite_f(av[j][e]) ? av[j][e] : 0.f;
                // products of the non-finite activations with the live weights, element by element
#pragma unroll
                for (int j = 0; j < RM; ++j)
#pragma unroll
                    for (int jn = 0; jn < RN; ++jn)
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int m = r0 + 32 * j + 8 * (q >> 2) + 4 * h + (q & 3);
                            if (m >= g.M || !cok[jn]) continue;
                            float add = 0.f;
                            for (int kk = k0; kk < min(k0 + 16, kend); ++kk) {
                                const float x = g.a[(long long)m * g.sam + (long long)kk * g.sak];
                                if (finite_f(x)) continue;
                                const int dki = g.sel ? g.dk[kk] : 0;
                                const bool live = g.sel == 0 || (g.sel == 1 ? dcol[jn] >= dki : dki >= dcol[jn]);
                                if (live) add += x * g.b[ocol[jn] * g.sbc + (long long)kk * g.sbk];
                            }
                            acc[j][jn][q] += add;
                        }
            }
        }
        if constexpr (MODE == 0) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int j = 0; j < RM; ++j)
#pragma unroll
                    for (int jn = 0; jn < RN; ++jn)
                        acc[j][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][s], bv[jn][s], acc[j][jn], 0, 0, 0);
        } else {
            bf16x8 ab[RM], bb[RN];
#pragma unroll
            for (int j = 0; j < RM; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) ab[j][e] = (__bf16)av[j][e];
#pragma unroll
            for (int jn = 0; jn < RN; ++jn)
#pragma unroll
                for (int e = 0; e < 8; ++e) bb[jn][e] = (__bf16)bv[jn][e];
#pragma unroll
            for (int j = 0; j < RM; ++j)
#pragma unroll
                for (int jn = 0; jn < RN; ++jn) acc[j][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[j], bb[jn], acc[j][jn], 0, 0, 0);
        }
    }

    // accumulator register q of a 32 x 32 block: row 8 (q / 4) + 4 h + q % 4, column r
    if constexpr (EPI == EPI_Y || EPI == EPI_WG) {
        float* y = g.y + (long long)blockIdx.z * g.zstride;
#pragma unroll
        for (int j = 0; j < RM; ++j)
#pragma unroll
            for (int jn = 0; jn < RN; ++jn) {
                if (!cok[jn]) continue;
                const int c = cw + 32 * jn + r;
                const float bsum = (EPI == EPI_Y && g.bias) ? g.bias[ocol[jn]] : 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int m = r0 + 32 * j + 8 * (q >> 2) + 4 * h + (q & 3);
                    if (m >= g.M) continue;
                    float v = acc[j][jn][q];
                    if (EPI == EPI_WG) {
                        if (g.dr[m] >= g.dc[c]) y[(long long)m * g.ldy + c] = v;       // masked entries are never written
                    } else {
                        v += bsum;
                        if (g.act) v = sigm(v);
                        y[(long long)m * g.ldy + c] = v;
                    }
                }
            }
    } else {
        // the head: the workgroup's 8 waves x 32 columns are the 256 classes of pixel blockIdx.x (RM = 4: 128 rows, RN = 1)
        static_assert(EPI != EPI_LSE || (WAVES == 8 && RN == 1), "one pixel per workgroup");
        const int d = blockIdx.x, cls = wave * 32 + r;
        const float bo = g.bias[(long long)d * 256 + cls];
        if constexpr (EPI == EPI_DL) {
            const float gs = g.scale * (g.gscale ? *g.gscale : 1.f);
#pragma unroll
            for (int j = 0; j < RM; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int m = r0 + 32 * j + 8 * (q >> 2) + 4 * h + (q & 3);
                    if (m >= g.M) continue;
                    const float L = g.lse[(long long)m * g.D + d];
                    const int t = made_target(g.img[(long long)m * g.D + d], g.normalize);
                    const float v = acc[j][0][q] + bo;
                    g.y[(long long)m * g.ldy + (long long)d * 256 + cls] = (expf(v - L) - (cls == t ? 1.f : 0.f)) * gs;
                }
        } else {
            __shared__ float smax[8][RM * 32], ssum[8][RM * 32], stgt[RM * 32], sred[RM * 32 / 64];
#pragma unroll
            for (int j = 0; j < RM; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int rl = 32 * j + 8 * (q >> 2) + 4 * h + (q & 3), m = r0 + rl;
                    const float v = acc[j][0][q] + bo;
                    float mx = v;
#pragma unroll
                    for (int off = 1; off < 32; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 32));
                    float s = expf(v - mx);
#pragma unroll
                    for (int off = 1; off < 32; off <<= 1) s += __shfl_xor(s, off, 32);
                    if (r == 0) { smax[wave][rl] = mx; ssum[wave][rl] = s; }
                    if (m < g.M && cls == made_target(g.img[(long long)m * g.D + d], g.normalize)) stgt[rl] = v;
                }
            __syncthreads();
            float nll = 0.f;
            if (threadIdx.x < RM * 32) {
                const int rl = threadIdx.x, m = r0 + rl;
                if (m < g.M) {
                    float mx = smax[0][rl];
#pragma unroll
                    for (int w = 1; w < 8; ++w) mx = fmaxf(mx, smax[w][rl]);
                    float s = 0.f;
#pragma unroll
                    for (int w = 0; w < 8; ++w) s += ssum[w][rl] * expf(smax[w][rl] - mx);
                    const float L = mx + logf(s);
                    g.lse[(long long)m * g.D + d] = L;
                    nll = L - stgt[rl];
                }
                for (int off = 32; off > 0; off >>= 1) nll += __shfl_xor(nll, off);
                if (lane == 0) sred[wave] = nll;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < RM * 32 / 64; ++w) t += sred[w];
                g.partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = t;
            }
        }
    }
}

// out[0] = scale * sum of partial[0 .. n) (one workgroup, fixed order)
__global__ __launch_bounds__(256) void made_reduce_kernel(int n, const float* __restrict__ partial, float scale, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1] + red[2] + red[3]) * scale;
}

// dx[m][c] = (sum over the S split-K slices) * s (1 - s), s = sv[m][c] (the sigmoid output of the layer below; null: no factor)
__global__ __launch_bounds__(256) void made_split_sum_kernel(int M, int C, int S, const float* __restrict__ part, const float* __restrict__ sv,
                                                             int lds, float* __restrict__ dx, int lddx) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * C) return;
    const int m = (int)(idx / C), c = (int)(idx - (long long)m * C);
    float t = 0.f;
    for (int z = 0; z < S; ++z) t += part[(long long)z * M * C + idx];
    if (sv) { const float s = sv[(long long)m * lds + c]; t *= s * (1.f - s); }
    dx[(long long)m * lddx + c] = t;
}

// out[c] = sum_m g[m][c] (bias gradients; written, fixed order)
__global__ __launch_bounds__(256) void made_colsum_kernel(int M, int C, const float* __restrict__ g, long long ld, float* __restrict__ out) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += g[(long long)m * ld + c];
    out[c] = s;
}

// One sampling step at position *counter of the H*W raster, one workgroup of 16 waves, a wave per (sample, channel) unit at a time.
// logits [N][C*256] are the head rows of the C units at that position.  The position is skipped only when no sample and no channel
// holds -1 there; otherwise every (sample, channel) gets a draw.
__global__ __launch_bounds__(1024) void made_sample_kernel(int N, int C, int HW, const float* __restrict__ logits, int* counter,
                                                           const float* __restrict__ uni, float* img, int normalize) {
    __shared__ int any_missing;
    const int pix = *counter;
    if (threadIdx.x == 0) any_missing = 0;
    __syncthreads();
    if (pix < HW)
        for (int i = threadIdx.x; i < N * C; i += blockDim.x)
            if (img[(size_t)i * HW + pix] == -1.f) any_missing = 1;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (pix < HW && any_missing) {
        for (int u = wave; u < N * C; u += nw) {
            const float* lr = logits + (size_t)u * 256;        // [n][c][256] = unit u = n * C + c
            float l[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) l[j] = lr[lane * 4 + j];
            const int k = ar_inverse_cdf_pick(l, uni[(size_t)pix * N * C + u], lane);
            if (lane == 0) {
                float v = (float)k / 255.f;
                if (normalize) v = v * 2.f - 1.f;
                img[(size_t)u * HW + pix] = v;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) counter[0] = pix + 1;
}

GemmArgs base_args(int M, int Nc, int K) {
    GemmArgs g{};
    g.M = M; g.Nc = Nc; g.K = K; g.kspan = K;
    return g;
}

template <int RM, int RN, int WAVES, int EPI, bool AKC, bool BKC>
int launch(int mode, const GemmArgs& g, int splits, hipStream_t st) {
    const dim3 grid((g.Nc + WAVES * RN * 32 - 1) / (WAVES * RN * 32), (g.M + RM * 32 - 1) / (RM * 32), splits);
    if (mode == MI_MADE_MODE_BF16) hipLaunchKernelGGL((made_gemm_kernel<1, RM, RN, WAVES, EPI, AKC, BKC>), grid, dim3(WAVES * 64), 0, st, g);
    else hipLaunchKernelGGL((made_gemm_kernel<0, RM, RN, WAVES, EPI, AKC, BKC>), grid, dim3(WAVES * 64), 0, st, g);
    return 0;
}

constexpr int HEAD_ROWS = 128;          // rows (samples) per head workgroup
constexpr int DGRAD_KSPAN = 2048;       // contraction slice of one split of the data gradient

bool mode_ok(int mode) { return mode == MI_MADE_MODE_FP32 || mode == MI_MADE_MODE_BF16; }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_made_supported(int D, int hidden, int C) {
    return D >= 1 && C >= 1 && C <= 4 && D % C == 0 && hidden >= 4 && hidden <= 8192 && hidden % 4 == 0 && (long long)D * 256 < (1ll << 30);
}

extern "C" int mi_made_linear(int mode, int N, int in, int out, const float* x, int ldx, const float* w, const float* b, const int* deg_in,
                              const int* deg_out, int act, float* y, int ldy, void* stream) {
    MI_REQUIRE(mode_ok(mode) && N >= 1 && in >= 1 && out >= 1, "bad mode or shape");
    MI_REQUIRE(x && w && b && deg_in && deg_out && y && ldx >= in && ldy >= out, "null operand or short pitch");
    GemmArgs g = base_args(N, out, in);
    g.a = x; g.sam = ldx; g.sak = 1;
    g.b = w; g.sbc = in; g.sbk = 1;
    g.dk = deg_in; g.dc = deg_out; g.sel = 1; g.fix = 1;
    g.bias = b; g.act = act; g.y = y; g.ldy = ldy;
    launch<1, 1, 4, EPI_Y, true, true>(mode, g, 1, ST);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mi_made_dgrad_workspace(int N, int in, int out) {
    return (size_t)((out + DGRAD_KSPAN - 1) / DGRAD_KSPAN) * N * in * sizeof(float);
}

extern "C" int mi_made_dgrad(int mode, int N, int in, int out, const float* gy, long long ldg, const float* w, const int* deg_in,
                             const int* deg_out, const float* s_in, int lds, float* work, float* dx, int lddx, void* stream) {
    MI_REQUIRE(mode_ok(mode) && N >= 1 && in >= 1 && out >= 1, "bad mode or shape");
    MI_REQUIRE(gy && w && deg_in && deg_out && work && dx && ldg >= out && lddx >= in && (!s_in || lds >= in), "null operand or short pitch");
    const int S = (out + DGRAD_KSPAN - 1) / DGRAD_KSPAN;
    GemmArgs g = base_args(N, in, out);
    g.a = gy; g.sam = ldg; g.sak = 1;
    g.b = w; g.sbc = 1; g.sbk = in;
    g.dk = deg_out; g.dc = deg_in; g.sel = 2;
    g.kspan = DGRAD_KSPAN; g.y = work; g.ldy = in; g.zstride = (long long)N * in;
    if (N > 64) launch<4, 1, 4, EPI_Y, true, false>(mode, g, S, ST);
    else launch<1, 1, 4, EPI_Y, true, false>(mode, g, S, ST);
    MI_LAUNCH_CHECK();
    const long long n = (long long)N * in;
    hipLaunchKernelGGL(made_split_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, N, in, S, (const float*)work, s_in, lds, dx, lddx);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_made_wgrad(int mode, int N, int in, int out, const float* gy, long long ldg, const float* x, int ldx, const int* deg_in,
                             const int* deg_out, float* dw, float* db, void* stream) {
    MI_REQUIRE(mode_ok(mode) && N >= 1 && in >= 1 && out >= 1, "bad mode or shape");
    MI_REQUIRE(gy && x && deg_in && deg_out && dw && db && ldg >= out && ldx >= in, "null operand or short pitch");
    GemmArgs g = base_args(out, in, N);
    g.a = gy; g.sam = 1; g.sak = ldg;
    g.b = x; g.sbc = 1; g.sbk = ldx;
    g.dr = deg_out; g.dc = deg_in; g.y = dw; g.ldy = in;
    launch<1, 4, 4, EPI_WG, false, false>(mode, g, 1, ST);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(made_colsum_kernel, dim3((out + 255) / 256), dim3(256), 0, ST, N, out, gy, ldg, db);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_made_head_partials(int N, int D) { return ((N + HEAD_ROWS - 1) / HEAD_ROWS) * D; }

static GemmArgs head_args(int N, int D, int Hd, const float* h, int ldh, const float* w, const float* b, const int* deg_in, const int* deg_out,
                          const float* img, int normalize) {
    GemmArgs g = base_args(N, D * 256, Hd);
    g.a = h; g.sam = ldh; g.sak = 1;
    g.b = w; g.sbc = Hd; g.sbk = 1;
    g.dk = deg_in; g.dc = deg_out; g.sel = 1;
    g.bias = b; g.img = img; g.D = D; g.normalize = normalize;
    return g;
}

extern "C" int mi_made_head_fwd(int mode, int N, int D, int Hd, const float* h, int ldh, const float* w, const float* b, const int* deg_in,
                                const int* deg_out, const float* img, int normalize, float* lse, float* partial, float* loss, void* stream) {
    MI_REQUIRE(mode_ok(mode) && N >= 1 && D >= 1 && Hd >= 1 && ldh >= Hd, "bad mode or shape");
    MI_REQUIRE(h && w && b && deg_in && deg_out && img && lse && partial && loss, "null operand");
    GemmArgs g = head_args(N, D, Hd, h, ldh, w, b, deg_in, deg_out, img, normalize);
    g.lse = lse; g.partial = partial;
    launch<4, 1, 8, EPI_LSE, true, true>(mode, g, 1, ST);
    MI_LAUNCH_CHECK();
    const float ln2 = 0.693147182464599609375f;                 // torch.log(torch.tensor(2.)) in fp32: the reference's `log2` buffer
    hipLaunchKernelGGL(made_reduce_kernel, dim3(1), dim3(256), 0, ST, mi_made_head_partials(N, D), (const float*)partial,
                       1.f / ((float)N * D * ln2), loss);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_made_head_dlogits(int mode, int N, int D, int Hd, const float* h, int ldh, const float* w, const float* b, const int* deg_in,
                                    const int* deg_out, const float* img, int normalize, const float* lse, const float* gscale, float* dl,
                                    void* stream) {
    MI_REQUIRE(mode_ok(mode) && N >= 1 && D >= 1 && Hd >= 1 && ldh >= Hd, "bad mode or shape");
    MI_REQUIRE(h && w && b && deg_in && deg_out && img && lse && dl, "null operand");
    GemmArgs g = head_args(N, D, Hd, h, ldh, w, b, deg_in, deg_out, img, normalize);
    g.lse = (float*)lse; g.gscale = gscale; g.y = dl; g.ldy = (long long)D * 256;
    const float ln2 = 0.693147182464599609375f;
    g.scale = 1.f / ((float)N * D * ln2);
    launch<4, 1, 8, EPI_DL, true, true>(mode, g, 1, ST);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_made_head_rows(int mode, int N, int C, int HW, int Hd, const float* h, int ldh, const float* w, const float* b,
                                 const int* deg_in, const int* deg_out, const int* pos, float* logits, void* stream) {
    MI_REQUIRE(mode_ok(mode) && N >= 1 && C >= 1 && HW >= 1 && Hd >= 1 && ldh >= Hd, "bad mode or shape");
    MI_REQUIRE(h && w && b && deg_in && deg_out && pos && logits, "null operand");
    GemmArgs g = base_args(N, C * 256, Hd);
    g.a = h; g.sam = ldh; g.sak = 1;
    g.b = w; g.sbc = Hd; g.sbk = 1;
    g.dk = deg_in; g.dc = deg_out; g.sel = 1; g.fix = 1;
    g.bias = b; g.y = logits; g.ldy = C * 256;
    g.pos = pos; g.remap_hw = HW;
    launch<1, 1, 4, EPI_Y, true, true>(mode, g, 1, ST);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_made_sample_step(int N, int C, int HW, const float* logits, int* counter, const float* uniforms, float* img, int normalize,
                                   void* stream) {
    MI_REQUIRE(N >= 1 && C >= 1 && C <= 4 && HW >= 1 && logits && counter && uniforms && img, "bad arguments");
    hipLaunchKernelGGL(made_sample_kernel, dim3(1), dim3(1024), 0, ST, N, C, HW, logits, counter, uniforms, img, normalize);
    MI_LAUNCH_CHECK();
    return 0;
}
