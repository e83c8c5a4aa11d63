// Latent discriminator of the FactorVAE family (reference src/networks/basic.py:64-112, MLPEncoder(L, [256, 256], 1) with its defaults):
//   x [N, L] -> Linear(L, 256) -> GroupNorm(1, 256) -> LeakyReLU(0.2) -> Linear(256, 256) -> BatchNorm1d(256) -> LeakyReLU(0.2)
//            -> Linear(256, 1) = logit [N],  loss = mean((logit - t)^2)  (src/utils/losses.py:12-17, "lsgan").
// About 4 MFLOP per pass at N = 64: launch-bound, so the whole network is two launches forward and three backward.  The one batch-wide
// dependency in each direction is BatchNorm's column statistics; everything else is local to a tile of RT rows.
//   forward   rows : x (formed on the fly from one of three sources) -> fc1 -> LayerNorm -> LeakyReLU -> fc2           (N / RT workgroups)
//             tail : column statistics, running statistics, BatchNorm -> LeakyReLU -> fc3, loss, mean logit             (1 workgroup)
//   backward  cols : head gradients and the two column sums BatchNorm's backward needs                                  (1 workgroup)
//             rows : d a2 -> fc2^T -> LeakyReLU' -> LayerNorm backward -> d a1 -> fc1^T = d x                           (N / RT workgroups)
//             params: fc2 / fc1 weight gradients and the remaining vectors, one output element per thread              (32 + L/8 + 1)
// Weights are stored input-major ([in][out]: thread = output column reads them coalesced).  Plain FMA, no matrix cores: at this size the
// arithmetic is a few microseconds of one CU.  Every tensor is fp32; every SUM (the contractions, the LayerNorm / BatchNorm statistics,
// the sums over the batch) is accumulated in fp64 and rounded once -- BatchNorm over N = 2 or 3 rows divides by the difference of two
// such sums, and the fp64 rate costs nothing here.  No atomics: every sum has a fixed order, two runs on the same inputs agree bit for
// bit.  Every element of every output is stored.
// A permutation index outside [0, N) makes its element 0 and is never used as an address.
// The row-tile steps up to fc2 and back down from it (staging, fc1, LayerNorm-1 both ways, both fc2 contractions, fc1^T, and the fc2 / fc1 /
// vector branches of the parameter kernel) are csrc/latent_mlp.h, shared with csrc/latent_disc_ln.hip.  Here are the input stage, the
// BatchNorm tail and head, the tape and the entry points.  This file keeps LayerNorm-1's statistics in fp32 (T = float in latent_mlp.h),
// as it shipped; the other file keeps them in fp64.
#include "latent_mlp.h"

namespace {

constexpr int TC = 16;
constexpr int NMAX = MI_LATENT_DISC_NMAX;

struct Src { const float* z; int ldz; const float* h; int ldh; const float* eps; const int64_t* perm; };
// tape (floats): xhat1 [N][H] | h1 [N][H] | a2 [N][H] | ln [N][2] (mean, rstd) | bn [2][H] (mean, rstd) as fp64 = 4 H floats | logit [N]
struct Tape { float *xhat1, *h1, *a2, *ln; double* bn; float* logit; };
// workspace of the backward (floats): da2 [N][H] | dn1 [N][H] | da1 [N][H] | cols [2][H] as fp64 = 4 H floats
struct Ws { float *da2, *dn1, *da1; double* cols; };
// BatchNorm runs in fp64 from the fp32 a2 in both directions (statistics, normalisation, and the backward's
// dn - mean(dn) - xhat mean(dn xhat), which for two or three rows cancels to a few parts in 1e5 of its terms).

__device__ __forceinline__ float load_x(const Src& s, int N, int L, int n, int j) {
    if (s.z) return s.z[(size_t)n * s.ldz + j];
    int m = n;
    if (s.perm) {
        const int64_t q = s.perm[(size_t)j * N + n];
        if (q < 0 || q >= (int64_t)N) return 0.f;
        m = (int)q;
    }
    return s.h[(size_t)m * s.ldh + j] + expf(s.h[(size_t)m * s.ldh + L + j]) * s.eps[(size_t)m * L + j];
}

// ------------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(TPB) void ld_fwd_rows(int N, int L, Src s, Par p, Tape t) {
    __shared__ float xs[RT][LMAX];
    __shared__ __align__(16) float hs[RT][LDP];
    __shared__ float st[RT][2];
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6;
    stage_rows(xs, r0, N, L, [=](int n, int j) { return load_x(s, N, L, n, j); });
    __syncthreads();
    float acc[RT];
    fc_in(xs, p.w1, p.b1, L, c, acc, hs);
    __syncthreads();
    ln_stats<float>(hs, st, lane, wv);
    __syncthreads();
    ln_act_store<float>(acc, st, p.g1[c], p.be1[c], r0, N, c, t.xhat1, t.h1, hs);
    if (c < RT && r0 + c < N) { t.ln[2 * (r0 + c)] = st[c][0]; t.ln[2 * (r0 + c) + 1] = st[c][1]; }
    __syncthreads();
    double a2[RT];
    fc256(hs, p.w2, (double)p.b2[c], c, a2);
#pragma unroll
    for (int r = 0; r < RT; ++r)
        if (r0 + r < N) t.a2[(size_t)(r0 + r) * H + c] = (float)a2[r];
}

// One workgroup, thread = column.  training: batch statistics (biased variance for normalising, unbiased into running_var).
__global__ __launch_bounds__(TPB) void ld_fwd_tail(int N, int training, float target, float momentum, Par p, Tape t, float* __restrict__ rmean,
                                                   float* __restrict__ rvar, int64_t* __restrict__ nbt, float* __restrict__ out3) {
    __shared__ float lg[NMAX];
    __shared__ float part[TC][H + 1];
    __shared__ double red[4];
    const int c = threadIdx.x;
    double mean, rstd;
    if (training) {
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += t.a2[(size_t)n * H + c];
        const double m = s / N;
        double ss = 0.0;
        for (int n = 0; n < N; ++n) { const double a = t.a2[(size_t)n * H + c] - m; ss = fma(a, a, ss); }
        mean = m;
        rstd = 1.0 / sqrt(ss / N + (double)EPS);
        if (rmean) {
            const double mo = momentum;
            rmean[c] = (float)((1.0 - mo) * rmean[c] + mo * m);
            rvar[c] = (float)((1.0 - mo) * rvar[c] + mo * (ss / (N - 1)));
        }
        if (nbt && c == 0) *nbt += 1;
    } else {
        mean = rmean[c];
        rstd = 1.0 / sqrt((double)rvar[c] + (double)EPS);
    }
    t.bn[c] = mean;
    t.bn[H + c] = rstd;
    const double g = p.g2[c], be = p.be2[c], w3 = p.w3[c], b3 = p.b3[0];
    const int rr = c >> 4, q = c & 15;
    for (int n0 = 0; n0 < N; n0 += TC) {
#pragma unroll 4
        for (int i = 0; i < TC; ++i) {
            float v = 0.f;
            if (n0 + i < N) v = (float)(leaky(fma(g, (t.a2[(size_t)(n0 + i) * H + c] - mean) * rstd, be)) * w3);
            part[i][c] = v;
        }
        __syncthreads();
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += part[rr][q * 16 + i];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (q == 0 && n0 + rr < N) lg[n0 + rr] = (float)(sum + b3);
        __syncthreads();
    }
    double sl = 0.0, sm = 0.0, sq = 0.0;
    for (int n = c; n < N; n += TPB) {
        const double v = lg[n], d = v - (double)target;
        t.logit[n] = lg[n];
        sl = fma(d, d, sl);
        sm += v;
        sq = fma(v, v, sq);
    }
    sl = block_sum_256d(sl, red);
    sm = block_sum_256d(sm, red);
    sq = block_sum_256d(sq, red);
    if (c == 0) { out3[0] = (float)(sl / N); out3[1] = (float)(sm / N); out3[2] = (float)(sq / N); }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// d loss / d logit[n] = 2 (logit[n] - target) / N.  One workgroup, thread = column: gradients of fc3 and of BatchNorm's affine pair,
// and the column sums of dn2 and dn2 * xhat2 that the row kernel needs.
__global__ __launch_bounds__(TPB) void ld_bwd_cols(int N, float target, Par p, Tape t, Ws w, Grad g, int want_params, float ps, int pacc) {
    const int c = threadIdx.x;
    const double mean = t.bn[c], rstd = t.bn[H + c], g2 = p.g2[c], be2 = p.be2[c], w3 = p.w3[c], k = 2.0 / N;
    double sdn = 0.0, sdx = 0.0, sw3 = 0.0, sdl = 0.0;
    for (int n = 0; n < N; ++n) {
        const double dl = k * ((double)t.logit[n] - (double)target);
        const double xh = (t.a2[(size_t)n * H + c] - mean) * rstd, pre = fma(g2, xh, be2);
        const double dn = dl * w3 * leaky_d(pre);
        sdn += dn;
        sdx = fma(dn, xh, sdx);
        sw3 = fma(dl, leaky(pre), sw3);
        sdl += dl;
    }
    w.cols[c] = sdn / N;
    w.cols[H + c] = sdx / N;
    if (want_params) {
        put(g.be2 + c, sdn, ps, pacc);
        put(g.g2 + c, sdx, ps, pacc);
        put(g.w3 + c, sw3, ps, pacc);
        if (c == 0) put(g.b3, sdl, ps, pacc);
    }
}

__global__ __launch_bounds__(TPB) void ld_bwd_rows(int N, int L, int training, float target, Par p, Tape t, Ws w, float* __restrict__ dz,
                                                   int lddz, float zs, int zacc) {
    __shared__ __align__(16) float ds[RT][LDP];
    __shared__ __align__(16) float xs[RT][LDP];
    __shared__ float st[RT][2];
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6;
    {
        const double mean = t.bn[c], rstd = t.bn[H + c], g2 = p.g2[c], be2 = p.be2[c], w3 = p.w3[c], k = 2.0 / N;
        const double mdn = w.cols[c], mdx = w.cols[H + c];                   // column means of dn2 and dn2 * xhat2
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            float v = 0.f;
            if (n < N) {
                const double dl = k * ((double)t.logit[n] - (double)target);
                const double xh = (t.a2[(size_t)n * H + c] - mean) * rstd;
                const double dn = dl * w3 * leaky_d(fma(g2, xh, be2));
                v = (float)(training ? g2 * rstd * ((dn - mdn) - xh * mdx) : g2 * rstd * dn);
                w.da2[(size_t)n * H + c] = v;
            }
            ds[r][c] = v;
        }
    }
    __syncthreads();
    double a0[RT];
    fc256_t(ds, p.w2, c, a0);
    float da1[RT];
    ln1_backward<float>(a0, p.g1[c], t.xhat1, t.h1, t.ln + 1, 2, r0, N, c, lane, wv, ds, xs, st, w.dn1, w.da1, da1);
    if (!dz) return;
    input_grad(da1, ds, p.w1, L, r0, N, c, dz, lddz, zs, zacc);
}

// d W2, d W1 and d b2, d gamma1, d beta1, d b1: the workgroups of params_common, and no others.
__global__ __launch_bounds__(TPB) void ld_bwd_params(int N, int L, Src s, Tape t, Ws w, Grad g, float ps, int pacc) {
    params_common(blockIdx.x, N, L, [=](int n, int j) { return load_x(s, N, L, n, j); }, t.h1, t.xhat1, w.da2, w.dn1, w.da1, g, ps, pacc);
}

inline Tape tape_of(float* base, int N) {
    Tape t;
    const size_t nh = (size_t)N * H;
    t.xhat1 = base; t.h1 = base + nh; t.a2 = base + 2 * nh; t.ln = base + 3 * nh;
    t.bn = reinterpret_cast<double*>(t.ln + 2 * (size_t)N);                  // 8-byte aligned: an even number of floats in front
    t.logit = t.ln + 2 * (size_t)N + 4 * H;
    return t;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_latent_disc_supported(int N, int L, int Hd) {
    if (Hd != H) return mi_set_error(0, "mi_latent_disc: hidden width %d (only 256 is built)", Hd), 0;
    if (L < 1 || L > LMAX) return mi_set_error(0, "mi_latent_disc: latent width %d outside [1, 64]", L), 0;
    if (N < 2 || N > NMAX) return mi_set_error(0, "mi_latent_disc: %d rows outside [2, %d] (BatchNorm1d needs 2 in training)", N, NMAX), 0;
    return 1;
}

extern "C" size_t mi_latent_disc_tape_floats(int N) { return N > 0 ? 3 * (size_t)N * H + 3 * (size_t)N + 4 * H : 0; }
extern "C" size_t mi_latent_disc_workspace_floats(int N) { return N > 0 ? 3 * (size_t)N * H + 4 * H : 0; }

static int ld_source(int N, int L, const float* z, int ldz, const float* h, int ldh, const float* eps, const int64_t* perm, Src* s) {
    if (z) {
        if (h || eps || perm || ldz < L) return -1;
    } else {
        if (!h || !eps || ldh < 2 * L) return -1;
    }
    s->z = z; s->ldz = ldz; s->h = h; s->ldh = ldh; s->eps = eps; s->perm = perm;
    (void)N;
    return 0;
}

extern "C" int mi_latent_disc_fwd(int N, int L, int Hd, const float* z, int ldz, const float* h, int ldh, const float* eps, const int64_t* perm,
                                  const float* const* params, int training, float target, float momentum, float* running_mean,
                                  float* running_var, int64_t* num_batches_tracked, float* tape, float* out3, void* stream) {
    MI_REQUIRE(mi_latent_disc_supported(N, L, Hd) == 1, "shape not supported (H == 256, 1 <= L <= 64, 2 <= N <= MI_LATENT_DISC_NMAX)");
    MI_REQUIRE(params && tape && out3, "bad argument");
    Src s;
    MI_REQUIRE(ld_source(N, L, z, ldz, h, ldh, eps, perm, &s) == 0, "input: either z (ldz >= L) or h + eps (ldh >= 2 L) [+ perm]");
    MI_REQUIRE(all_ten_set(params), "a parameter pointer is null");
    MI_REQUIRE(training || (running_mean && running_var), "evaluation mode needs the running statistics");
    MI_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
    MI_REQUIRE(aligned16(tape), "tape: 16-byte alignment");
    const Par p = par_of(params);
    Tape t = tape_of(tape, N);
    hipLaunchKernelGGL(ld_fwd_rows, dim3((N + RT - 1) / RT), dim3(TPB), 0, ST, N, L, s, p, t);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_fwd_tail, dim3(1), dim3(TPB), 0, ST, N, training ? 1 : 0, target, momentum, p, t, running_mean, running_var,
                       training ? num_batches_tracked : nullptr, out3);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_latent_disc_bwd(int N, int L, int Hd, const float* z, int ldz, const float* h, int ldh, const float* eps, const int64_t* perm,
                                  const float* const* params, int training, float target, const float* tape, float* workspace,
                                  float* const* grads, float param_scale, int accumulate_params, float* dz, int lddz, float dz_scale,
                                  int accumulate_dz, void* stream) {
    MI_REQUIRE(mi_latent_disc_supported(N, L, Hd) == 1, "shape not supported (H == 256, 1 <= L <= 64, 2 <= N <= MI_LATENT_DISC_NMAX)");
    MI_REQUIRE(params && tape && workspace, "bad argument");
    MI_REQUIRE(grads || dz, "neither parameter gradients nor an input gradient asked for");
    Src s;
    MI_REQUIRE(ld_source(N, L, z, ldz, h, ldh, eps, perm, &s) == 0, "input: either z (ldz >= L) or h + eps (ldh >= 2 L) [+ perm]");
    MI_REQUIRE(!dz || (!perm && lddz >= L), "dz: lddz >= L, and no input gradient through a permutation");
    MI_REQUIRE(all_ten_set(params) && (!grads || all_ten_set(grads)), "a parameter / gradient pointer is null");
    MI_REQUIRE(aligned16(tape) && aligned16(workspace) && aligned16(params[0]) && aligned16(params[4]), "tape, workspace, fc1 / fc2 weights: 16-byte alignment");
    const Par p = par_of(params);
    const Grad g = grad_of(grads);
    Tape t = tape_of(const_cast<float*>(tape), N);
    Ws w;
    const size_t nh = (size_t)N * H;
    w.da2 = workspace; w.dn1 = workspace + nh; w.da1 = workspace + 2 * nh; w.cols = reinterpret_cast<double*>(workspace + 3 * nh);
    hipLaunchKernelGGL(ld_bwd_cols, dim3(1), dim3(TPB), 0, ST, N, target, p, t, w, g, grads ? 1 : 0, param_scale, accumulate_params ? 1 : 0);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_bwd_rows, dim3((N + RT - 1) / RT), dim3(TPB), 0, ST, N, L, training ? 1 : 0, target, p, t, w, dz, lddz, dz_scale,
                       accumulate_dz ? 1 : 0);
    MI_LAUNCH_CHECK();
    if (grads) {
        hipLaunchKernelGGL(ld_bwd_params, dim3(NB_W2 + (L + KT - 1) / KT + 1), dim3(TPB), 0, ST, N, L, s, t, w, g, param_scale,
                           accumulate_params ? 1 : 0);
        MI_LAUNCH_CHECK();
    }
    return 0;
}
