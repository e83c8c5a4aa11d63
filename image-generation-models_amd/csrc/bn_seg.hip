// Segmented BatchNorm + activation, and the adversarial losses of the plain GAN (reference src/models/gan.py, src/utils/losses.py:4-24).
//
// A GAN's discriminator phase runs the discriminator on the real batch and on the fake batch, each with its own batch statistics and
// its own running-statistics update.  Here both halves go through as ONE tensor of S segments of M rows: statistics per (segment,
// channel), the running statistics updated S times in segment order, the activation folded into the normalisation pass and its
// backward folded into both backward passes (the masked gradient is never written).
//
// Two launches each way, no atomics, no zero-on-entry workspace, no grid-wide sync, no "last workgroup" counter:
//   1. sums    grid (P, S): workgroup (p, s) walks rows [p R, (p + 1) R) of segment s and STORES its two fp64 sums per channel into
//              slot (s, p) of the workspace: [S][P][2][C] doubles, every element written on every call;
//   2. apply   grid (G, S): every workgroup first adds the P partials of its segment's channels in the order p = 0 .. P - 1 (each
//              workgroup gets the same bits), then streams its rows.  Workgroup (0, s) writes mean / rstd of segment s; workgroup
//              (0, 0) also walks all S segments in order with one thread per channel for the running statistics (forward) or for
//              dgamma / dbeta (backward).
// P and R depend on (M, C) alone, so two runs give the same bits.  fp32 tensors, fp64 sums (E[x^2] - mean^2 keeps its digits at a
// mean of 1e3 and a spread of 1), 16-byte loads and stores per lane.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BNS_PMAX = 64;          // most partials per segment: what every apply workgroup adds up per channel
constexpr int BNS_QUADS = 1024;       // channel quads an apply workgroup streams (4 per thread)

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_LEAKY = 2 };

__host__ __device__ inline int bns_rows_per_wg(int M, int C) {
    const int r0 = 64 * (C >= 256 ? 1 : 256 / C);                   // bn_sums_kernel's share
    const int r1 = (M + BNS_PMAX - 1) / BNS_PMAX;
    return r0 > r1 ? r0 : r1;
}
inline int bns_partials(int M, int C) { const int R = bns_rows_per_wg(M, C); return (M + R - 1) / R; }
inline int bns_apply_rows(int C) { const int r = BNS_QUADS / (C / 4); return r > 0 ? r : 1; }

__device__ __forceinline__ float act_f(float v, int act, float slope) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_LEAKY) return v > 0.f ? v : v * slope;
    return v;
}
// gradient through the activation from its OUTPUT y (mi_relu_bwd / mi_leaky_relu_bwd)
__device__ __forceinline__ float act_grad_f(float y, float g, int act, float slope) {
    if (act == ACT_RELU) return y > 0.f ? g : 0.f;
    if (act == ACT_LEAKY) return y > 0.f ? g : g * slope;
    return g;
}

// part[(s P + p)][0][c] = sum_rows a, [1][c] = sum_rows a * b.  Forward: a = b = x.  Backward (BWD): a = act'(y) dy, b = xhat.
// Thread = (channel quad q, row lane rl), as bn_sums_kernel.
template <bool BWD>
__global__ __launch_bounds__(256) void bn_seg_sums_kernel(int M, int C, int R, const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ dy, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, int act, float slope, double* __restrict__ part) {
    __shared__ double red[2][256][4];
    const int Q = C / 4, t = threadIdx.x, s = blockIdx.y, p = blockIdx.x, P = gridDim.x;
    const int lanes = 256 / Q;                                       // Q <= 256
    const int q = t % Q, rl = t / Q;
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = {1.f, 1.f, 1.f, 1.f};
    if (BWD) { mu = *reinterpret_cast<const f32x4*>(mean + (size_t)s * C + 4 * q); rs = *reinterpret_cast<const f32x4*>(rstd + (size_t)s * C + 4 * q); }
    const int r0 = p * R, r1 = min(M, r0 + R);
    const size_t base = (size_t)s * M * C + 4 * q;
    for (int r = r0 + rl; r < r1; r += lanes) {
        const size_t o = base + (size_t)r * C;
        f32x4 av = *reinterpret_cast<const f32x4*>(x + o), bv = av;
        if (BWD) {
            bv = (av - mu) * rs;
            const f32x4 yv = *reinterpret_cast<const f32x4*>(y + o), gv = *reinterpret_cast<const f32x4*>(dy + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) av[j] = act_grad_f(yv[j], gv[j], act, slope);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { s0[j] += (double)av[j]; s1[j] += (double)av[j] * (double)bv[j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[0][t][j] = s0[j]; red[1][t][j] = s1[j]; }
    __syncthreads();
    if (t < Q) {
        double* out = part + ((size_t)s * P + p) * 2 * C;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v0 = 0, v1 = 0;
            for (int k = t; k < lanes * Q; k += Q) { v0 += red[0][k][j]; v1 += red[1][k][j]; }
            out[4 * t + j] = v0;
            out[C + 4 * t + j] = v1;
        }
    }
}

// the two totals of (segment s, channel c): the P partials in the order p = 0 .. P - 1
__device__ __forceinline__ void bns_total(const double* __restrict__ part, int s, int P, int C, int c, double& a, double& b) {
    const double* p0 = part + (size_t)s * P * 2 * C + c;
    double v0 = 0, v1 = 0;
    for (int p = 0; p < P; ++p) { v0 += p0[(size_t)p * 2 * C]; v1 += p0[(size_t)p * 2 * C + C]; }
    a = v0; b = v1;
}

// y = act(gamma (x - mean_s) rstd_s + beta).  training: mean / rstd from the partials; else from the running statistics.
__global__ __launch_bounds__(256) void bn_seg_apply_kernel(int M, int C, int S, int P, int rows, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           float momentum, float eps, int training, int act, float slope,
                                                           const double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[2][1024];
    const int t = threadIdx.x, s = blockIdx.y, Q = C / 4;
    for (int c = t; c < C; c += 256) {
        float m, r;
        if (training) {
            double a, b;
            bns_total(part, s, P, C, c, a, b);
            const double mu = a / M, var = fmax(b / M - mu * mu, 0.0);
            m = (float)mu;
            r = (float)(1.0 / sqrt(var + (double)eps));
        } else {
            m = running_mean[c];
            r = rsqrtf(running_var[c] + eps);
        }
        sm[0][c] = m; sm[1][c] = r;
        if (blockIdx.x == 0) { mean[(size_t)s * C + c] = m; rstd[(size_t)s * C + c] = r; }
    }
    if (training && blockIdx.x == 0 && s == 0 && (running_mean || running_var)) {
        // the S momentum updates of channel c, segment 0 first: this thread alone touches running_*[c]
        for (int c = t; c < C; c += 256) {
            float rm = running_mean ? running_mean[c] : 0.f, rv = running_var ? running_var[c] : 0.f;
            for (int k = 0; k < S; ++k) {
                double a, b;
                bns_total(part, k, P, C, c, a, b);
                const double mu = a / M, var = fmax(b / M - mu * mu, 0.0);
                rm = (1.f - momentum) * rm + momentum * (float)mu;
                rv = (1.f - momentum) * rv + momentum * (float)(M > 1 ? var * M / (M - 1) : var);
            }
            if (running_mean) running_mean[c] = rm;
            if (running_var) running_var[c] = rv;
        }
    }
    __syncthreads();
    const int r0 = blockIdx.x * rows, r1 = min(M, r0 + rows);
    const size_t base = ((size_t)s * M + r0) * Q;
    const int nq = (r1 - r0) * Q;                                    // 256 % Q == 0: a thread keeps its channel quad
    const int q = t % Q;
    const f32x4 mu = *reinterpret_cast<const f32x4*>(&sm[0][4 * q]), rs = *reinterpret_cast<const f32x4*>(&sm[1][4 * q]);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * q), b = *reinterpret_cast<const f32x4*>(beta + 4 * q);
    const f32x4* xin = reinterpret_cast<const f32x4*>(x) + base;
    f32x4* yout = reinterpret_cast<f32x4*>(y) + base;
    for (int i = t; i < nq; i += 256) {
        f32x4 v = (xin[i] - mu) * rs * g + b;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_f(v[j], act, slope);
        yout[i] = v;
    }
}

// dx = gamma rstd_s (g - S0_s / M - xhat S1_s / M), g = act'(y) dy;  dgamma (+)= sum_s S1_s, dbeta (+)= sum_s S0_s
__global__ __launch_bounds__(256) void bn_seg_bwd_apply_kernel(int M, int C, int S, int P, int rows, const float* __restrict__ x,
                                                               const float* __restrict__ y, const float* dy,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, float* dx, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int accumulate, int act, float slope,
                                                               const double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[2][1024];
    const int t = threadIdx.x, s = blockIdx.y, Q = C / 4;
    for (int c = t; c < C; c += 256) {
        double a, b;
        bns_total(part, s, P, C, c, a, b);
        sm[0][c] = (float)(a / M); sm[1][c] = (float)(b / M);
    }
    if (blockIdx.x == 0 && s == 0 && (dgamma || dbeta)) {
        for (int c = t; c < C; c += 256) {
            double ta = 0, tb = 0;
            for (int k = 0; k < S; ++k) {
                double a, b;
                bns_total(part, k, P, C, c, a, b);
                ta += a; tb += b;
            }
            if (dbeta) dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)ta;
            if (dgamma) dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)tb;
        }
    }
    __syncthreads();
    const int r0 = blockIdx.x * rows, r1 = min(M, r0 + rows);
    const size_t base = ((size_t)s * M + r0) * Q;
    const int nq = (r1 - r0) * Q;
    const int q = t % Q;
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(&sm[0][4 * q]), s1 = *reinterpret_cast<const f32x4*>(&sm[1][4 * q]);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)s * C + 4 * q), rs = *reinterpret_cast<const f32x4*>(rstd + (size_t)s * C + 4 * q);
    const f32x4 gr = *reinterpret_cast<const f32x4*>(gamma + 4 * q) * rs;
    const f32x4* xin = reinterpret_cast<const f32x4*>(x) + base;
    const f32x4* yin = reinterpret_cast<const f32x4*>(y) + base;
    const f32x4* gin = reinterpret_cast<const f32x4*>(dy) + base;
    f32x4* out = reinterpret_cast<f32x4*>(dx) + base;
    for (int i = t; i < nq; i += 256) {
        const f32x4 xh = (xin[i] - mu) * rs, yv = yin[i];
        f32x4 gv = gin[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = act_grad_f(yv[j], gv[j], act, slope);
        out[i] = gr * (gv - s0 - xh * s1);
    }
}

struct AdvTargets { int real[8]; };

// One workgroup.  Per segment: loss = mean f(x), mean logit, dlogit = scale f'(x) / M; every element in fp64, sums in a fixed order.
//   vanilla  f = softplus(-x) (real) | softplus(x) (fake), written as max(-+x, 0) + log1p(exp(-|x|)): finite at |x| = 200
//   lsgan    f = (x - 1)^2 | x^2
//   hinge    f = max(1 - x, 1) | max(1 + x, 0): the REFERENCE's formula (losses.py:17-21), not the textbook hinge max(1 - x, 0);
//            a tie of torch.maximum's two operands sends half the gradient each way, as torch does
//   wasserstein (mode 3)  f = -x | +x: the WGAN critic's loss (src/models/wgan.py), dlogit = -+scale / M
__global__ __launch_bounds__(256) void adv_loss_kernel(int S, int M, int mode, AdvTargets tg, float scale, const float* __restrict__ logit,
                                                       int ld, float* __restrict__ loss, float* __restrict__ mean_logit,
                                                       float* __restrict__ dlogit, int lddl) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    for (int s = 0; s < S; ++s) {
        const bool real = tg.real[s] != 0;
        double sl = 0, sx = 0;
        for (int i = t; i < M; i += 256) {
            const double x = (double)logit[((size_t)s * M + i) * ld];
            double f, d;
            if (mode == 0) {
                const double e = exp(-fabs(x)), sg = x >= 0 ? 1.0 / (1.0 + e) : e / (1.0 + e);      // sigmoid(x)
                const double sgn = x >= 0 ? e / (1.0 + e) : 1.0 / (1.0 + e);                        // sigmoid(-x)
                f = fmax(real ? -x : x, 0.0) + log1p(e);
                d = real ? -sgn : sg;
            } else if (mode == 1) {
                const double u = x - (real ? 1.0 : 0.0);
                f = u * u; d = 2.0 * u;
            } else if (mode == 3) {
                f = real ? -x : x; d = real ? -1.0 : 1.0;
            } else if (real) {
                f = fmax(1.0 - x, 1.0); d = x < 0 ? -1.0 : (x == 0 ? -0.5 : 0.0);
            } else {
                f = fmax(1.0 + x, 0.0); d = x > -1.0 ? 1.0 : (x == -1.0 ? 0.5 : 0.0);
            }
            sl += f; sx += x;
            if (dlogit) dlogit[((size_t)s * M + i) * lddl] = (float)((double)scale * d / M);
        }
        red[0][t] = sl; red[1][t] = sx;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; }
            __syncthreads();
        }
        if (t == 0) { loss[s] = (float)(red[0][0] / M); mean_logit[s] = (float)(red[1][0] / M); }
        __syncthreads();
    }
}

}  // namespace

#define ST ((hipStream_t)stream)
#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

static bool bns_ok(int S, int M, int C) {
    return S >= 1 && S <= 65535 && M > 0 && C >= 4 && C % 4 == 0 && C <= 1024 && 256 % (C / 4 > 256 ? 256 : C / 4) == 0 &&
           (size_t)S * M * (C / 4) < ((size_t)1 << 40);
}

extern "C" int mi_bn_seg_rows_per_workgroup(int M, int C) { return (M > 0 && C >= 4 && C <= 1024) ? bns_rows_per_wg(M, C) : 0; }

extern "C" size_t mi_bn_seg_workspace(int S, int M, int C) {
    if (!bns_ok(S, M, C)) return 0;
    return (size_t)S * bns_partials(M, C) * 2 * C * sizeof(double);
}

extern "C" int mi_bn_seg_fwd(int S, int M, int C, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                             float* running_mean, float* running_var, float momentum, float eps, int training, int act, float slope,
                             void* ws, void* stream) {
    MI_REQUIRE(bns_ok(S, M, C), "needs S >= 1, M >= 1, C % 4 == 0, C/4 a power of two <= 256");
    MI_REQUIRE(x && gamma && beta && y && mean && rstd && AL16(x) && AL16(y) && AL16(gamma) && AL16(beta) && AL16(mean) && AL16(rstd),
               "needs 16-byte aligned dense tensors");
    MI_REQUIRE(y != x, "y must not alias x: the backward reads x");
    MI_REQUIRE(act >= ACT_NONE && act <= ACT_LEAKY, "act: 0 none, 1 relu, 2 leaky relu");
    const int P = bns_partials(M, C), rows = bns_apply_rows(C);
    if (training) {
        MI_REQUIRE(ws && (((uintptr_t)ws) & 7) == 0, "training mode needs the workspace (8-byte aligned)");
        hipLaunchKernelGGL(bn_seg_sums_kernel<false>, dim3(P, S), dim3(256), 0, ST, M, C, bns_rows_per_wg(M, C), x, nullptr, nullptr, nullptr,
                           nullptr, 0, 0.f, (double*)ws);
    } else {
        MI_REQUIRE(running_mean && running_var, "evaluation mode needs the running statistics");
    }
    hipLaunchKernelGGL(bn_seg_apply_kernel, dim3((M + rows - 1) / rows, S), dim3(256), 0, ST, M, C, S, P, rows, x, gamma, beta, y, mean, rstd,
                       running_mean, running_var, momentum, eps, training, act, slope, (const double*)ws);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_bn_seg_bwd(int S, int M, int C, const float* x, const float* mean, const float* rstd, const float* gamma, const float* y,
                             const float* dy, float* dx, float* dgamma, float* dbeta, int accumulate, int act, float slope, void* ws,
                             void* stream) {
    MI_REQUIRE(bns_ok(S, M, C), "needs S >= 1, M >= 1, C % 4 == 0, C/4 a power of two <= 256");
    MI_REQUIRE(x && mean && rstd && gamma && y && dy && dx && AL16(x) && AL16(y) && AL16(dy) && AL16(dx) && AL16(gamma) && AL16(mean) && AL16(rstd),
               "needs 16-byte aligned dense tensors");
    MI_REQUIRE(dx != x && dx != y, "dx may alias dy only");
    MI_REQUIRE(act >= ACT_NONE && act <= ACT_LEAKY, "act: 0 none, 1 relu, 2 leaky relu");
    MI_REQUIRE(ws && (((uintptr_t)ws) & 7) == 0, "needs the workspace (8-byte aligned)");
    const int P = bns_partials(M, C), rows = bns_apply_rows(C);
    hipLaunchKernelGGL(bn_seg_sums_kernel<true>, dim3(P, S), dim3(256), 0, ST, M, C, bns_rows_per_wg(M, C), x, y, dy, mean, rstd, act, slope,
                       (double*)ws);
    hipLaunchKernelGGL(bn_seg_bwd_apply_kernel, dim3((M + rows - 1) / rows, S), dim3(256), 0, ST, M, C, S, P, rows, x, y, dy, mean, rstd, gamma, dx,
                       dgamma, dbeta, accumulate, act, slope, (const double*)ws);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_adv_loss(int S, int M, int mode, const int* target_is_real, float scale, const float* logit, int ld, float* loss,
                           float* mean_logit, float* dlogit, int lddl, void* stream) {
    MI_REQUIRE(S >= 1 && S <= 8 && M >= 1 && (size_t)S * M < ((size_t)1 << 28), "needs 1 <= S <= 8 segments of M >= 1 logits");
    MI_REQUIRE(mode >= 0 && mode <= 3, "mode: 0 vanilla, 1 lsgan, 2 hinge, 3 wasserstein");
    MI_REQUIRE(target_is_real && logit && loss && mean_logit, "null pointer");
    MI_REQUIRE(ld >= 1 && (!dlogit || lddl >= 1), "ld, lddl: element strides >= 1");
    AdvTargets tg = {};
    for (int s = 0; s < S; ++s) tg.real[s] = target_is_real[s];
    hipLaunchKernelGGL(adv_loss_kernel, dim3(1), dim3(256), 0, ST, S, M, mode, tg, scale, logit, ld, loss, mean_logit, dlogit, lddl);
    MI_LAUNCH_CHECK();
    return 0;
}
