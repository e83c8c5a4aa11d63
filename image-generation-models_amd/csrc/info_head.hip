// The InfoGAN's heads on the shared feature (reference src/models/info_gan.py:37-43, 64-74, 99-133) and its structured generator input:
//   f [S*M, E] (the common layer's output, read in place with a pitch)
//   a     = LeakyReLU(f, 0.01)                                  never stored: the backward recomputes it from f
//   logit = a w_d + b_d                                         netD = Sequential(LeakyReLU(), Linear(E, 1))
//   q1    = LeakyReLU(a W1 + b1, 0.01),  q = q1 W2 + b2         netQ = Sequential(LeakyReLU(), Linear(E, 128), LeakyReLU(), Linear(128, Dd V + Cc))
// The slope is torch's default 0.01, not the conv nets' 0.2.  q's first Dd V columns are [V][Dd] (column v Dd + d is value v of code d,
// the layout of the reference's flattened [N, V, Dd] one-hot), its last Cc columns the continuous codes.
//   forward   rows   : a tile of RT rows per workgroup, thread c = hidden column c: logit, q1, q, the loss terms of each row, dlogit, dq
//             reduce : one workgroup: the adversarial loss and the mean logit per segment, the cross-entropy, the MSE (6 numbers)
//   backward  rows   : dq1 = leaky'(q1) (dq W2^T), df = leaky'(f) (dlogit w_d + dq1 W1^T)
//             params : dW1, db1, dW2, db2 and / or dw_d, db_d, one output element per thread, rows walked upward
// Conventions as csrc/latent_mlp.h: weights input-major, plain FMA, every tensor fp32, every sum fp64 in a fixed order and rounded
// once, no atomics, every element of every output stored, the workspace needs no zeroing.  Row n is computed by the same instruction
// sequence whichever tile and segment it falls into.
#include "common.h"

namespace {

constexpr int HQ = 128, TPB = 128, RT = 4, KC = 256, QMAX = 64, EMAX = 4096, KT = 8;
constexpr float SLOPE = 0.01f;

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }
__device__ __forceinline__ float leaky_d(float v) { return v > 0.f ? 1.f : SLOPE; }
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

struct Par { const float *wd, *bd, *w1, *b1, *w2, *b2; };
struct Grad { float *wd, *bd, *w1, *b1, *w2, *b2; };
struct Code { int Dd, V, Cc; const long long* idx; const float* cont; int ldc; float lambda; };

// ------------------------------------------------------------------------------------------------------------------ latent
// out[n] = [one-hot of the Dd codes, column v Dd + d | cont_c | z | 0 ...]; an index outside [0, V) leaves its code's columns 0.
__global__ __launch_bounds__(256) void info_latent_kernel(int N, int Dd, int V, int Cc, int Nz, const long long* __restrict__ idx,
                                                          const float* __restrict__ cont, int ldc, const float* __restrict__ z, int ldz,
                                                          float* __restrict__ out, int ld) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * ld) return;
    const int n = (int)(i / ld), j = (int)(i - (size_t)n * ld), dv = Dd * V;
    float v = 0.f;
    if (j < dv) {
        const int val = j / Dd, d = j - val * Dd;
        v = idx[(size_t)n * Dd + d] == (long long)val ? 1.f : 0.f;
    } else if (j < dv + Cc) {
        v = cont[(size_t)n * ldc + (j - dv)];
    } else if (j < dv + Cc + Nz) {
        v = z[(size_t)n * ldz + (j - dv - Cc)];
    }
    out[i] = v;
}

// ------------------------------------------------------------------------------------------------------------------ forward
// ws [rows][4] doubles: adversarial loss of the row, its logit, sum_d cross-entropy, sum_c squared error.
// logit null: no D head; with_q without cd.idx: the Q head's outputs alone (q, and q1 where asked for), no losses.
__global__ __launch_bounds__(TPB) void info_fwd_rows(int S, int M, int E, const float* __restrict__ f, int ldf, Par p, float t0, float t1,
                                                     float scale, int with_q, Code cd, float* __restrict__ logit, float* __restrict__ dlogit,
                                                     float* __restrict__ q1, float* __restrict__ q, float* __restrict__ dq,
                                                     double* __restrict__ ws) {
    __shared__ __align__(16) float as[RT][KC];
    __shared__ __align__(16) float q1s[RT][HQ];
    __shared__ float qs[RT][QMAX];
    __shared__ double part[RT][QMAX];
    const int rows = S * M, c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6;
    const bool with_d = logit != nullptr;                                    // uniform over the grid, like with_q and cd.idx
    double acc[RT], lg[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) { acc[r] = with_q ? (double)p.b1[c] : 0.0; lg[r] = 0.0; }
    for (int k0 = 0; k0 < E; k0 += KC) {
        const int len = min(KC, E - k0);                                     // a multiple of 4
        __syncthreads();
        for (int i = c; i < RT * KC; i += TPB) {
            const int r = i / KC, k = i - r * KC, n = r0 + r;
            as[r][k] = (n < rows && k < len) ? leaky(f[(size_t)n * ldf + k0 + k]) : 0.f;
        }
        __syncthreads();
        if (with_q) {
            for (int k = 0; k < len; k += 4) {
                const float* w = p.w1 + (size_t)(k0 + k) * HQ + c;
                const double w0 = w[0], w1 = w[HQ], w2 = w[2 * HQ], w3 = w[3 * HQ];
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const float4 a = *reinterpret_cast<const float4*>(&as[r][k]);
                    acc[r] = fma((double)a.w, w3, fma((double)a.z, w2, fma((double)a.y, w1, fma((double)a.x, w0, acc[r]))));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {                                       // the D head: wave wv owns rows wv, wv + 2
            if (!with_d || (r & 1) != wv) continue;
            double s = 0.0;
            for (int k = lane; k < len; k += 64) s = fma((double)as[r][k], (double)p.wd[k0 + k], s);
            lg[r] += wave_sum_d(s);
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int n = r0 + r;
        if (!with_d || (r & 1) != wv || lane != 0 || n >= rows) continue;
        const float lgf = (float)(lg[r] + (double)p.bd[0]);
        const double x = lgf, t = n < M ? t0 : t1;
        const double e = exp(-fabs(x));                                      // in (0, 1]: no overflow at either end
        logit[n] = lgf;
        ws[(size_t)n * 4 + 0] = fmax(x, 0.0) - x * t + log1p(e);
        ws[(size_t)n * 4 + 1] = x;
        dlogit[n] = (float)((double)scale / M * ((x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - t));
    }
    if (!with_q) return;                                                     // uniform over the grid
    const int Qd = cd.Dd * cd.V + cd.Cc, dv = cd.Dd * cd.V;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const float v = leaky((float)acc[r]);
        q1s[r][c] = v;
        if (q1 && r0 + r < rows) q1[(size_t)(r0 + r) * HQ + c] = v;
    }
    __syncthreads();
    for (int o = c; o < RT * Qd; o += TPB) {
        const int r = o / Qd, j = o - r * Qd;
        double s = p.b2[j];
        for (int k = 0; k < HQ; ++k) s = fma((double)q1s[r][k], (double)p.w2[(size_t)k * Qd + j], s);
        const float v = (float)s;
        qs[r][j] = v;
        if (r0 + r < rows) q[(size_t)(r0 + r) * Qd + j] = v;
    }
    if (!cd.idx) return;
    __syncthreads();
    // cross-entropy of code d of row r over its V values (columns v Dd + d), mean over rows * Dd
    for (int o = c; o < RT * cd.Dd; o += TPB) {
        const int r = o / cd.Dd, d = o - r * cd.Dd, n = r0 + r;
        double ce = 0.0;
        if (n < rows) {
            double m = qs[r][d];
            for (int v = 1; v < cd.V; ++v) m = fmax(m, (double)qs[r][v * cd.Dd + d]);
            double s = 0.0;
            for (int v = 0; v < cd.V; ++v) s += exp((double)qs[r][v * cd.Dd + d] - m);
            const double lse = m + log(s);
            const long long tg = cd.idx[(size_t)n * cd.Dd + d];
            const double k = (double)cd.lambda / ((double)rows * cd.Dd);
            ce = lse - ((tg >= 0 && tg < cd.V) ? (double)qs[r][(int)tg * cd.Dd + d] : 0.0);
            for (int v = 0; v < cd.V; ++v)
                dq[(size_t)n * Qd + v * cd.Dd + d] = (float)(k * (exp((double)qs[r][v * cd.Dd + d] - lse) - (tg == (long long)v ? 1.0 : 0.0)));
        }
        part[r][d] = ce;
    }
    for (int o = c; o < RT * cd.Cc; o += TPB) {
        const int r = o / cd.Cc, j = o - r * cd.Cc, n = r0 + r;
        double se = 0.0;
        if (n < rows) {
            const double diff = (double)qs[r][dv + j] - (double)cd.cont[(size_t)n * cd.ldc + j];
            se = diff * diff;
            dq[(size_t)n * Qd + dv + j] = (float)((double)cd.lambda * 2.0 * diff / ((double)rows * cd.Cc));
        }
        part[r][cd.Dd + j] = se;                                             // Dd + Cc <= Dd V + Cc <= QMAX
    }
    __syncthreads();
    if (c < RT && r0 + c < rows) {
        double ce = 0.0, se = 0.0;
        for (int d = 0; d < cd.Dd; ++d) ce += part[c][d];
        for (int j = 0; j < cd.Cc; ++j) se += part[c][cd.Dd + j];
        ws[(size_t)(r0 + c) * 4 + 2] = ce;
        ws[(size_t)(r0 + c) * 4 + 3] = se;
    }
}

// One workgroup: out6 = adversarial loss of segment 0, of segment 1, mean logit of segment 0, of segment 1, cross-entropy, MSE.
// Thread c sums rows c, c + 256, ... upward, then the block sum: a fixed order.  What was not asked for is stored as 0.
__global__ __launch_bounds__(256) void info_fwd_reduce(int S, int M, int with_d, int with_q, int Dd, int Cc, const double* __restrict__ ws,
                                                       float* __restrict__ out6) {
    __shared__ double red[4];
    const int c = threadIdx.x, rows = S * M;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = c; n < rows; n += 256) {
        const int s = n < M ? 0 : 1;
        if (with_d) { v[s] += ws[(size_t)n * 4 + 0]; v[2 + s] += ws[(size_t)n * 4 + 1]; }
        if (with_q) { v[4] += ws[(size_t)n * 4 + 2]; v[5] += ws[(size_t)n * 4 + 3]; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = block_sum_256d(v[i], red);
    if (c == 0) {
        const double im = 1.0 / M;
        out6[0] = (float)(v[0] * im);
        out6[1] = (float)(v[1] * im);
        out6[2] = (float)(v[2] * im);
        out6[3] = (float)(v[3] * im);
        out6[4] = with_q ? (float)(v[4] / ((double)rows * Dd)) : 0.f;
        out6[5] = with_q ? (float)(v[5] / ((double)rows * Cc)) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// dq1w [rows][128] (nullable): what the parameter kernel reads.  df nullable.
__global__ __launch_bounds__(TPB) void info_bwd_rows(int rows, int E, int Qd, const float* __restrict__ f, int ldf, Par p,
                                                     const float* __restrict__ dlogit, const float* __restrict__ q1,
                                                     const float* __restrict__ dq, float* __restrict__ df, int lddf, float* __restrict__ dq1w) {
    __shared__ __align__(16) float d1s[RT][HQ];
    __shared__ float dqs[RT][QMAX];
    __shared__ float dls[RT];
    const int c = threadIdx.x, r0 = blockIdx.x * RT;
    if (c < RT) dls[c] = (r0 + c < rows) ? dlogit[r0 + c] : 0.f;
    if (dq) {
        for (int o = c; o < RT * Qd; o += TPB) {
            const int r = o / Qd, j = o - r * Qd;
            dqs[r][j] = (r0 + r < rows) ? dq[(size_t)(r0 + r) * Qd + j] : 0.f;
        }
        __syncthreads();
        double a[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) a[r] = 0.0;
        for (int j = 0; j < Qd; ++j) {
            const double w = p.w2[(size_t)c * Qd + j];
#pragma unroll
            for (int r = 0; r < RT; ++r) a[r] = fma((double)dqs[r][j], w, a[r]);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            float v = 0.f;
            if (n < rows) {
                v = (float)(a[r] * (double)leaky_d(q1[(size_t)n * HQ + c]));   // sign(q1) = sign of the pre-activation
                if (dq1w) dq1w[(size_t)n * HQ + c] = v;
            }
            d1s[r][c] = v;
        }
    }
    __syncthreads();
    if (!df) return;
    for (int e = c; e < E; e += TPB) {
        double a[RT];
        const double w = p.wd[e];
#pragma unroll
        for (int r = 0; r < RT; ++r) a[r] = (double)dls[r] * w;
        if (dq) {
            const float* wr = p.w1 + (size_t)e * HQ;
            for (int k = 0; k < HQ; k += 4) {
                const float4 w4 = *reinterpret_cast<const float4*>(wr + k);
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const float4 d = *reinterpret_cast<const float4*>(&d1s[r][k]);
                    a[r] = fma((double)d.w, (double)w4.w, fma((double)d.z, (double)w4.z, fma((double)d.y, (double)w4.y, fma((double)d.x, (double)w4.x, a[r]))));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            if (n < rows) df[(size_t)n * lddf + e] = (float)(a[r] * (double)leaky_d(f[(size_t)n * ldf + e]));
        }
    }
}

// Workgroups, in this order.  With the Q gradients: E / KT.. for dW1 [e0 .. e0+KT)[c] (ceil), Qd for dW2 [c][j], 1 for db1 and db2.
// With the D-head gradients: ceil(E / TPB) for dw_d, 1 for db_d.  Every sum walks the rows upward.
__global__ __launch_bounds__(TPB) void info_bwd_params(int rows, int E, int Qd, int nq, const float* __restrict__ f, int ldf,
                                                       const float* __restrict__ dlogit, const float* __restrict__ q1,
                                                       const float* __restrict__ dq, const float* __restrict__ dq1w, Grad g) {
    const int c = threadIdx.x, nb1 = (E + KT - 1) / KT;
    int b = blockIdx.x;
    if (b < nq) {
        if (b < nb1) {
            const int e0 = b * KT;
            double acc[KT];
#pragma unroll
            for (int i = 0; i < KT; ++i) acc[i] = 0.0;
            for (int n = 0; n < rows; ++n) {
                const double d = dq1w[(size_t)n * HQ + c];
                const float* fr = f + (size_t)n * ldf + e0;
#pragma unroll
                for (int i = 0; i < KT; ++i)
                    if (e0 + i < E) acc[i] = fma((double)leaky(fr[i]), d, acc[i]);
            }
#pragma unroll
            for (int i = 0; i < KT; ++i)
                if (e0 + i < E) g.w1[(size_t)(e0 + i) * HQ + c] = (float)acc[i];
        } else if (b < nb1 + Qd) {
            const int j = b - nb1;
            double acc = 0.0;
            for (int n = 0; n < rows; ++n) acc = fma((double)q1[(size_t)n * HQ + c], (double)dq[(size_t)n * Qd + j], acc);
            g.w2[(size_t)c * Qd + j] = (float)acc;
        } else {
            double a1 = 0.0, a2 = 0.0;
            for (int n = 0; n < rows; ++n) {
                a1 += dq1w[(size_t)n * HQ + c];
                if (c < Qd) a2 += dq[(size_t)n * Qd + c];
            }
            g.b1[c] = (float)a1;
            if (c < Qd) g.b2[c] = (float)a2;
        }
        return;
    }
    b -= nq;
    const int nbd = (E + TPB - 1) / TPB;
    if (b < nbd) {
        const int e = b * TPB + c;
        if (e >= E) return;
        double acc = 0.0;
        for (int n = 0; n < rows; ++n) acc = fma((double)leaky(f[(size_t)n * ldf + e]), (double)dlogit[n], acc);
        g.wd[e] = (float)acc;
    } else if (c == 0) {
        double acc = 0.0;
        for (int n = 0; n < rows; ++n) acc += dlogit[n];
        g.bd[0] = (float)acc;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_info_latent(int N, int Dd, int V, int Cc, int Nz, const long long* dis_c_index, const float* cont_c, int ldc, const float* z,
                              int ldz, float* out, int ld, void* stream) {
    MI_REQUIRE(N >= 1 && Dd >= 1 && V >= 1 && Cc >= 1 && Nz >= 0, "N, Dd, V, Cc >= 1 and Nz >= 0");
    MI_REQUIRE((long long)Dd * V + Cc + Nz <= (1 << 20), "latent wider than 2^20");
    MI_REQUIRE(dis_c_index && cont_c && out && (z || Nz == 0), "null pointer");
    MI_REQUIRE(ldc >= Cc && (Nz == 0 || ldz >= Nz) && ld >= Dd * V + Cc + Nz, "ldc >= Cc, ldz >= Nz, ld >= Dd V + Cc + Nz");
    const size_t total = (size_t)N * ld;
    hipLaunchKernelGGL(info_latent_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST, N, Dd, V, Cc, Nz, dis_c_index, cont_c, ldc,
                       z, ldz, out, ld);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_info_head_supported(int S, int M, int E, int Hd, int Dd, int V, int Cc) {
    if (Hd != HQ) return mi_set_error(0, "mi_info_head: hidden width %d (only 128 is built)", Hd), 0;
    if (E < 4 || E > EMAX || E % 4 != 0) return mi_set_error(0, "mi_info_head: feature width %d (a multiple of 4 in [4, 4096])", E), 0;
    if (S < 1 || S > 2 || M < 1 || (long long)S * M > (1 << 24))
        return mi_set_error(0, "mi_info_head: %d segments of %d rows (1 or 2 segments of at least 1 row, 2^24 rows at the most)", S, M), 0;
    if (Dd == 0 && V == 0 && Cc == 0) return 1;                              // the D head alone
    if (Dd < 1 || V < 1 || Cc < 1 || (long long)Dd * V + Cc > QMAX)
        return mi_set_error(0, "mi_info_head: codes Dd=%d, V=%d, Cc=%d (each at least 1, Dd V + Cc <= 64)", Dd, V, Cc), 0;
    return 1;
}

extern "C" size_t mi_info_head_workspace_doubles(int rows) { return rows > 0 ? 4 * (size_t)rows : 0; }

extern "C" int mi_info_head_fwd(int S, int M, int E, int Hd, const float* f, int ldf, const float* const* params, int target0_is_real,
                                int target1_is_real, float scale, int Dd, int V, int Cc, const long long* dis_c_index, const float* cont_c,
                                int ldc, float lambda_I, float* logit, float* dlogit, float* q1, float* q, float* dq, double* ws, float* out6,
                                void* stream) {
    const int with_d = logit != nullptr, with_q = q != nullptr, with_loss = with_q && dis_c_index != nullptr;
    MI_REQUIRE(with_d || with_q, "neither the D head (logit) nor the Q head (q) asked for");
    MI_REQUIRE(mi_info_head_supported(S, M, E, Hd, with_loss ? Dd : 0, with_loss ? V : 0, with_loss ? Cc : 0) == 1, "shape not supported");
    MI_REQUIRE(f && ldf >= E && params, "null pointer or ldf < E");
    MI_REQUIRE(with_d ? (params[0] && params[1] && dlogit && ws && out6) : !dlogit, "the D head needs w_d, b_d, logit, dlogit, ws and out6");
    Code cd = {};
    if (with_q) {
        MI_REQUIRE(params[2] && params[3] && params[4] && params[5], "the Q head needs its four parameters");
        if (with_loss) {
            MI_REQUIRE(cont_c && q1 && dq && ws && out6 && ldc >= Cc, "the Q losses need dis_c_index, cont_c (ldc >= Cc), q1, dq, ws and out6");
        } else {
            MI_REQUIRE(!cont_c && !dq, "the Q head without losses: dis_c_index, cont_c and dq all null");
            MI_REQUIRE(Dd >= 0 && V >= 0 && Cc >= 0 && (long long)Dd * V + Cc >= 1 && (long long)Dd * V + Cc <= QMAX, "Qd = Dd V + Cc in [1, 64]");
        }
        cd = Code{Dd, V, Cc, with_loss ? dis_c_index : nullptr, cont_c, ldc, lambda_I};
    }
    const Par p = {params[0], params[1], params[2], params[3], params[4], params[5]};
    const int rows = S * M;
    hipLaunchKernelGGL(info_fwd_rows, dim3((rows + RT - 1) / RT), dim3(TPB), 0, ST, S, M, E, f, ldf, p, target0_is_real ? 1.f : 0.f,
                       target1_is_real ? 1.f : 0.f, scale, with_q, cd, logit, dlogit, q1, q, dq, ws);
    MI_LAUNCH_CHECK();
    if (with_d || with_loss) {
        hipLaunchKernelGGL(info_fwd_reduce, dim3(1), dim3(256), 0, ST, S, M, with_d, with_loss, Dd, Cc, ws, out6);
        MI_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mi_info_head_bwd(int S, int M, int E, int Hd, int Qd, const float* f, int ldf, const float* const* params, const float* dlogit,
                                const float* q1, const float* dq, float* df, int lddf, float* dq1_ws, float* const* grads, void* stream) {
    const int with_q = dq != nullptr;
    MI_REQUIRE(mi_info_head_supported(S, M, E, Hd, 0, 0, 0) == 1, "shape not supported");
    MI_REQUIRE(!with_q || (Qd >= 2 && Qd <= QMAX), "Qd = Dd V + Cc in [2, 64]");
    MI_REQUIRE(f && ldf >= E && params && params[0] && dlogit, "null pointer or ldf < E");
    MI_REQUIRE(!with_q || (q1 && params[2] && params[4] && aligned16(params[2])), "the Q head needs q1, W1 (16-byte aligned) and W2");
    MI_REQUIRE(!df || lddf >= E, "df: lddf >= E");
    const bool gq = grads && (grads[2] || grads[3] || grads[4] || grads[5]), gd = grads && (grads[0] || grads[1]);
    MI_REQUIRE(df || gq || gd, "neither a feature gradient nor parameter gradients asked for");
    MI_REQUIRE(!gq || (with_q && grads[2] && grads[3] && grads[4] && grads[5] && dq1_ws), "Q gradients: all four, with dq and the dq1 workspace");
    MI_REQUIRE(!gd || (grads[0] && grads[1]), "D-head gradients: both");
    const Par p = {params[0], params[1], params[2], params[3], params[4], params[5]};
    const int rows = S * M;
    if (df || gq) {
        hipLaunchKernelGGL(info_bwd_rows, dim3((rows + RT - 1) / RT), dim3(TPB), 0, ST, rows, E, Qd, f, ldf, p, dlogit, q1, dq, df, lddf,
                           gq ? dq1_ws : nullptr);
        MI_LAUNCH_CHECK();
    }
    if (gq || gd) {
        const Grad g = {grads[0], grads[1], grads[2], grads[3], grads[4], grads[5]};
        const int nq = gq ? (E + KT - 1) / KT + Qd + 1 : 0, nd = gd ? (E + TPB - 1) / TPB + 1 : 0;
        hipLaunchKernelGGL(info_bwd_params, dim3(nq + nd), dim3(TPB), 0, ST, rows, E, Qd, nq, f, ldf, dlogit, q1, dq, dq1_ws, g);
        MI_LAUNCH_CHECK();
    }
    return 0;
}
