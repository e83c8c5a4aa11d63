// Pair head of BiGAN's discriminator (reference src/models/BiGAN.py:100-126): everything of D(x, z) but dis_x's conv trunk.
//   dis_z    code [.., L] -> Linear(L, H) -> GroupNorm(1, H) -> LeakyReLU -> Linear(H, H) -> BatchNorm1d(H) -> LeakyReLU -> Linear(H, H) -> LeakyReLU = zf
//   dis_pair cat(zf, xf) [.., 2H] -> Linear(2H, H) -> GroupNorm(1, H) -> LeakyReLU -> Linear(H, 1) = logit          (xf: dis_x's output rows)
// on 2 N rows as two segments (0: real = (imgs, encoder(imgs)), 1: fake = (decoder(z), z)), which is the reference's two calls of D: BatchNorm1d
// keeps statistics per segment and updates its running statistics twice, segment 0 first.  The adversarial losses of both optimizers
// (g_loss: real against False + fake against True; d_loss: the opposite targets; src/utils/losses.py:4-24) and their derivatives by the
// logits come out of the forward.  The concat is never written: fc4 walks zf from LDS and xf from its own pitched rows.
//   forward   a    : code -> fc1 -> LayerNorm -> LeakyReLU -> fc2 = a2, per-tile column sums of a2 and a2^2 per segment      (2N / RT workgroups)
//             b    : the sums in slot order -> BatchNorm -> LeakyReLU -> fc3 -> LeakyReLU -> fc4 -> LayerNorm -> LeakyReLU -> fc5 = logit,
//                    dlogit_g, dlogit_d, per-tile loss sums; workgroup 0 updates the running statistics                    (2N / RT workgroups)
//             tail : the loss sums in slot order -> six scalars                                                               (1 workgroup)
//   backward  a    : dlogit -> fc5^T -> LayerNorm-4 backward -> fc4^T = (d zf, d xf) -> fc3^T -> d of BatchNorm's output, its column sums
//             b    : the sums in slot order -> BatchNorm backward -> fc2^T -> LayerNorm-1 backward -> fc1^T = d code (segment 0 only)
//             params: the sixteen parameter gradients, one output element per thread, every sum over the rows upward
// The backward is linear in dlogit.  Its two right-hand sides -- dlogit_g for the input gradients, dlogit_d for the parameter gradients --
// go down the same launches one after the other: a call that asks for both launches what a call for the parameters alone launches, and a
// right-hand side's results do not depend on whether the other one was asked for.
// Conventions of the family (csrc/latent_mlp.h): a workgroup owns a tile of RT rows, thread c owns hidden column c (TPB = H), weights
// input-major, plain FMA, every tensor fp32, every SUM accumulated in fp64 in a fixed order and rounded once, no atomics, every element
// of every output stored, a workspace that needs no zeroing.  Two runs agree bit for bit.  H is a template parameter; 128 is instantiated.
// The helpers here are the H-parametrised forms of latent_mlp.h's, with the LayerNorm statistics kept in fp64 (its T = double).
#include "common.h"

namespace {

constexpr int RT = 8, KT = 8, LMAX = 128;
constexpr float SLOPE = 0.2f, EPS = 1e-5f;

struct Par { const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3, *wp, *bp, *gp, *bep, *wc, *bc; };
struct Grad { float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3, *wp, *bp, *gp, *bep, *wc, *bc; };
// e: segment 0's code rows, z: segment 1's, xf: dis_x's 2N output rows
struct In { int N, L; const float* e; int lde; const float* z; int ldz; const float* xf; int ldf; };

inline Par par_of(const float* const* q) {
    return Par{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15]};
}
inline Grad grad_of(float* const* q) {
    return q ? Grad{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15]} : Grad{};
}
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// tape (floats), M = 2N rows: xhat1 | h1 | a2 | a3 | xhat4 | h4 (each [M][H]) | rstd1 [M] | rstd4 [M] | bn [2 segments][mean, rstd][H] as fp64
template <int H> struct Tape {
    float *xhat1, *h1, *a2, *a3, *xhat4, *h4, *rstd1, *rstd4;
    double* bn;
    explicit Tape(float* b, int M) {
        const size_t mh = (size_t)M * H;
        xhat1 = b; h1 = b + mh; a2 = b + 2 * mh; a3 = b + 3 * mh; xhat4 = b + 4 * mh; h4 = b + 5 * mh;
        rstd1 = b + 6 * mh; rstd4 = rstd1 + M;
        bn = reinterpret_cast<double*>(rstd4 + M);                       // M is even: 8-byte aligned
    }
};
template <int H> size_t tape_floats(int M) { return 6 * (size_t)M * H + 2 * (size_t)M + 8 * H; }

// workspace (floats), T = ceil(M / RT) tiles:
//   cols  fp64 [2][T][2 segments][2][H]   forward: [0] holds the sums of a2, a2^2; backward: per right-hand side the sums of dn2, dn2 xhat2
//   loss  fp64 [T][2 segments][4]         forward: sums of the g-side loss, the d-side loss and the logit
//   dn2   [2 right-hand sides][M][H]      d of BatchNorm's output through LeakyReLU'
//   dn4 | da4 | da3 | da2 | dn1 | da1     each [M][H]: what the parameter kernel reads (the parameter right-hand side only)
template <int H> struct Ws {
    double *cols, *loss;
    float *dn2, *dn4, *da4, *da3, *da2, *dn1, *da1;
    int T;
    explicit Ws(float* b, int M) {
        T = (M + RT - 1) / RT;
        const size_t mh = (size_t)M * H;
        cols = reinterpret_cast<double*>(b);
        loss = cols + (size_t)8 * T * H;
        dn2 = b + (size_t)16 * T * H + (size_t)16 * T;
        dn4 = dn2 + 2 * mh; da4 = dn4 + mh; da3 = da4 + mh; da2 = da3 + mh; dn1 = da2 + mh; da1 = dn1 + mh;
    }
    __device__ __forceinline__ double* col(int q, int t, int s, int k) const { return cols + ((((size_t)q * T + t) * 2 + s) * 2 + k) * H; }
};
template <int H> size_t ws_floats(int M) { const size_t T = (M + RT - 1) / RT; return 16 * T * H + 16 * T + 8 * (size_t)M * H; }

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }
__device__ __forceinline__ float leaky_d(float v) { return v > 0.f ? 1.f : SLOPE; }
__device__ __forceinline__ double leaky(double v) { return v > 0.0 ? v : (double)SLOPE * v; }
__device__ __forceinline__ double leaky_d(double v) { return v > 0.0 ? 1.0 : (double)SLOPE; }

__device__ __forceinline__ void put(float* p, double v, float scale, int accumulate) {
    *p = (float)(accumulate ? fma((double)scale, v, (double)*p) : (double)scale * v);
}

__device__ __forceinline__ float load_code(const In& in, int n, int j) {
    return n < in.N ? in.e[(size_t)n * in.lde + j] : in.z[(size_t)(n - in.N) * in.ldz + j];
}

// acc[r] = bias + sum_k hs[r][k] W[k][c] (W input-major, pitch H), k upward; `acc` continues a chain when first is false
template <int H> __device__ __forceinline__ void fc(const float (*hs)[H + 4], const float* __restrict__ w, double bias, int c, double* acc, bool first) {
    if (first) {
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r] = bias;
    }
    for (int k = 0; k < H; k += 4) {
        const double w0 = w[(size_t)k * H + c], w1 = w[(size_t)(k + 1) * H + c];
        const double w2 = w[(size_t)(k + 2) * H + c], w3 = w[(size_t)(k + 3) * H + c];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float4 hv = *reinterpret_cast<const float4*>(&hs[r][k]);
            acc[r] = fma((double)hv.w, w3, fma((double)hv.z, w2, fma((double)hv.y, w1, fma((double)hv.x, w0, acc[r]))));
        }
    }
}

// the transpose: acc[r] = sum_k ds[r][k] W[row][k], along row `row` of the [in][out] weights
template <int H> __device__ __forceinline__ void fc_t(const float (*ds)[H + 4], const float* w, int row, double* acc) {
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = 0.0;
    for (int k = 0; k < H; k += 4) {
        const float4 wv4 = *reinterpret_cast<const float4*>(&w[(size_t)row * H + k]);
        const double w0 = wv4.x, w1 = wv4.y, w2 = wv4.z, w3 = wv4.w;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float4 d = *reinterpret_cast<const float4*>(&ds[r][k]);
            acc[r] = fma((double)d.w, w3, fma((double)d.z, w2, fma((double)d.y, w1, fma((double)d.x, w0, acc[r]))));
        }
    }
}

// st[r] = (mean, rstd) of the RT rows in hs: one wave per row at a time, two passes, H / 64 elements per lane
template <int H> __device__ __forceinline__ void ln_stats(const float (*hs)[H + 4], double (*st)[2], int lane, int wv) {
    constexpr int E = H / 64, NW = H / 64;
    for (int r = wv; r < RT; r += NW) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < E; ++i) s += (double)hs[r][E * lane + i];
        const double m = wave_sum_d(s) * (1.0 / H);
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < E; ++i) { const double a = (double)hs[r][E * lane + i] - m; q = fma(a, a, q); }
        q = wave_sum_d(q) * (1.0 / H);
        if (lane == 0) { st[r][0] = m; st[r][1] = 1.0 / sqrt(q + (double)EPS); }
    }
}

// the two row means LayerNorm's backward needs: st[r] = (mean(d), mean(d * x))
template <int H> __device__ __forceinline__ void ln_bwd_stats(const float (*ds)[H + 4], const float (*xs)[H + 4], double (*st)[2], int lane, int wv) {
    constexpr int E = H / 64, NW = H / 64;
    for (int r = wv; r < RT; r += NW) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const double d = ds[r][E * lane + i];
            s1 += d;
            s2 = fma(d, (double)xs[r][E * lane + i], s2);
        }
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        if (lane == 0) { st[r][0] = s1 * (1.0 / H); st[r][1] = s2 * (1.0 / H); }
    }
}

// LayerNorm backward of the tile, from dxh = d xhat and xr = xhat (both 0 for rows from M on) to out[r] = d of the norm's input; stored
// in keep [M][H] as well unless that is null.  ds / xs must be free (a barrier behind their last reader); out may be dxh.
template <int H> __device__ __forceinline__ void ln_backward(const float* dxh, const float* xr, const float* rstd, int r0, int M, int c, int lane, int wv,
                                                             float (*ds)[H + 4], float (*xs)[H + 4], double (*st)[2], float* keep, float* out) {
#pragma unroll
    for (int r = 0; r < RT; ++r) { ds[r][c] = dxh[r]; xs[r][c] = xr[r]; }
    __syncthreads();
    ln_bwd_stats<H>(ds, xs, st, lane, wv);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int n = r0 + r;
        float v = 0.f;
        if (n < M) {
            v = (float)((double)rstd[n] * (((double)dxh[r] - st[r][0]) - (double)xr[r] * st[r][1]));
            if (keep) keep[(size_t)n * H + c] = v;
        }
        out[r] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ forward
template <int H> __global__ __launch_bounds__(H) void pd_fwd_a(In in, Par p, Tape<H> t, Ws<H> w) {
    __shared__ float xs[RT][LMAX];
    __shared__ __align__(16) float hs[RT][H + 4];
    __shared__ double st[RT][2];
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6, M = 2 * in.N, L = in.L;
    for (int i = c; i < RT * L; i += H) {
        const int r = i / L, j = i - r * L;
        xs[r][j] = (r0 + r < M) ? load_code(in, r0 + r, j) : 0.f;
    }
    __syncthreads();
    float a1[RT];
    {
        double a[RT];
        const double b = p.b1[c];
#pragma unroll
        for (int r = 0; r < RT; ++r) a[r] = b;
        for (int j = 0; j < L; ++j) {
            const double wj = p.w1[(size_t)j * H + c];
#pragma unroll
            for (int r = 0; r < RT; ++r) a[r] = fma((double)xs[r][j], wj, a[r]);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) { a1[r] = (float)a[r]; hs[r][c] = a1[r]; }
    }
    __syncthreads();
    ln_stats<H>(hs, st, lane, wv);
    __syncthreads();
    {
        const float g = p.g1[c], be = p.be1[c];
        float hv[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float xh = (float)(((double)a1[r] - st[r][0]) * st[r][1]);
            hv[r] = leaky(fmaf(g, xh, be));
            if (r0 + r < M) {
                t.xhat1[(size_t)(r0 + r) * H + c] = xh;
                t.h1[(size_t)(r0 + r) * H + c] = hv[r];
            }
        }
        if (c < RT && r0 + c < M) t.rstd1[r0 + c] = (float)st[c][1];
        __syncthreads();                                                     // the statistics pass is done reading hs
#pragma unroll
        for (int r = 0; r < RT; ++r) hs[r][c] = hv[r];
    }
    __syncthreads();
    double a2[RT];
    fc<H>(hs, p.w2, (double)p.b2[c], c, a2, true);
    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int n = r0 + r;
        if (n < M) {
            const float v = (float)a2[r];
            t.a2[(size_t)n * H + c] = v;
            const int s = n >= in.N;
            s1[s] += (double)v;
            s2[s] = fma((double)v, (double)v, s2[s]);
        }
    }
    for (int s = 0; s < 2; ++s) { w.col(0, blockIdx.x, s, 0)[c] = s1[s]; w.col(0, blockIdx.x, s, 1)[c] = s2[s]; }
}

// the adversarial loss f and f' of one logit against a target (csrc/bn_seg.hip, adv_loss_kernel: the same formulas)
__device__ __forceinline__ void adv(int mode, bool real, double x, double* f, double* d) {
    if (mode == 0) {
        const double e = exp(-fabs(x)), sg = x >= 0 ? 1.0 / (1.0 + e) : e / (1.0 + e), sgn = x >= 0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
        *f = fmax(real ? -x : x, 0.0) + log1p(e);
        *d = real ? -sgn : sg;
    } else if (mode == 1) {
        const double u = x - (real ? 1.0 : 0.0);
        *f = u * u; *d = 2.0 * u;
    } else if (real) {
        *f = fmax(1.0 - x, 1.0); *d = x < 0 ? -1.0 : (x == 0 ? -0.5 : 0.0);
    } else {
        *f = fmax(1.0 + x, 0.0); *d = x > -1.0 ? 1.0 : (x == -1.0 ? 0.5 : 0.0);
    }
}

template <int H> __global__ __launch_bounds__(H) void pd_fwd_b(In in, Par p, Tape<H> t, Ws<H> w, int training, int mode, float momentum,
                                                               float* __restrict__ rmean, float* __restrict__ rvar, int64_t* __restrict__ nbt,
                                                               float* __restrict__ logit, float* __restrict__ dlg, float* __restrict__ dld) {
    __shared__ __align__(16) float hs[RT][H + 4];
    __shared__ __align__(16) float fs[RT][H + 4];
    __shared__ double st[RT][2];
    __shared__ double red[RT][H / 64];
    __shared__ double lp[RT][3];
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6, N = in.N, M = 2 * N;
    double mean[2], rstd[2];
    if (training) {
        double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
        for (int i = 0; i < w.T; ++i)
            for (int s = 0; s < 2; ++s) { s1[s] += w.col(0, i, s, 0)[c]; s2[s] += w.col(0, i, s, 1)[c]; }
        double var[2];
        for (int s = 0; s < 2; ++s) {
            mean[s] = s1[s] / N;
            var[s] = fmax(s2[s] / N - mean[s] * mean[s], 0.0);
            rstd[s] = 1.0 / sqrt(var[s] + (double)EPS);
        }
        if (blockIdx.x == 0 && rmean) {                                      // two updates, segment 0 first: what two calls do
            const double mo = momentum;
            float rm = rmean[c], rv = rvar[c];
            for (int s = 0; s < 2; ++s) {
                rm = (float)((1.0 - mo) * rm + mo * mean[s]);
                rv = (float)((1.0 - mo) * rv + mo * (var[s] * N / (N - 1)));
            }
            rmean[c] = rm; rvar[c] = rv;
        }
        if (blockIdx.x == 0 && nbt && c == 0) *nbt += 2;
    } else {
        mean[0] = mean[1] = rmean[c];
        rstd[0] = rstd[1] = 1.0 / sqrt((double)rvar[c] + (double)EPS);
    }
    if (blockIdx.x == 0)
        for (int s = 0; s < 2; ++s) { t.bn[(2 * s) * H + c] = mean[s]; t.bn[(2 * s + 1) * H + c] = rstd[s]; }
    {
        const double g = p.g2[c], be = p.be2[c];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            float v = 0.f, f = 0.f;
            if (n < M) {
                const int s = n >= N;
                v = (float)leaky(fma(g, ((double)t.a2[(size_t)n * H + c] - mean[s]) * rstd[s], be));
                f = in.xf[(size_t)n * in.ldf + c];
            }
            hs[r][c] = v;
            fs[r][c] = f;
        }
    }
    __syncthreads();
    double acc[RT];
    fc<H>(hs, p.w3, (double)p.b3[c], c, acc, true);
    __syncthreads();                                                         // every thread is done reading h2
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const float a3 = (float)acc[r];
        if (r0 + r < M) t.a3[(size_t)(r0 + r) * H + c] = a3;
        hs[r][c] = r0 + r < M ? leaky(a3) : 0.f;
    }
    __syncthreads();
    fc<H>(hs, p.wp, (double)p.bp[c], c, acc, true);                          // the concat's first half: zf
    fc<H>(fs, p.wp + (size_t)H * H, 0.0, c, acc, false);                     // and its second: xf
    __syncthreads();
    float a4[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) { a4[r] = (float)acc[r]; hs[r][c] = a4[r]; }
    __syncthreads();
    ln_stats<H>(hs, st, lane, wv);
    __syncthreads();
    {
        const float g = p.gp[c], be = p.bep[c];
        const double wc = p.wc[c];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float xh = (float)(((double)a4[r] - st[r][0]) * st[r][1]);
            const float hv = leaky(fmaf(g, xh, be));
            if (r0 + r < M) {
                t.xhat4[(size_t)(r0 + r) * H + c] = xh;
                t.h4[(size_t)(r0 + r) * H + c] = hv;
            }
            const double v = wave_sum_d((double)hv * wc);
            if (lane == 0) red[r][wv] = v;
        }
        if (c < RT && r0 + c < M) t.rstd4[r0 + c] = (float)st[c][1];
    }
    __syncthreads();
    if (c < RT) {
        const int n = r0 + c;
        double fg = 0.0, fd = 0.0, x = 0.0;
        if (n < M) {
            double s = 0.0;
            for (int i = 0; i < H / 64; ++i) s += red[c][i];
            const float lg = (float)(s + (double)p.bc[0]);
            const bool real = n < N;
            double dg, dd;
            x = lg;
            adv(mode, !real, x, &fg, &dg);                                   // g_loss: real pairs against False, fake pairs against True
            adv(mode, real, x, &fd, &dd);
            logit[n] = lg;
            dlg[n] = (float)(dg / N);
            dld[n] = (float)(dd / N);
        }
        lp[c][0] = fg; lp[c][1] = fd; lp[c][2] = x;
    }
    __syncthreads();
    if (c < 6) {
        const int s = c / 3, k = c - 3 * s;
        double sum = 0.0;
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            if (n < M && (n >= N) == (s == 1)) sum += lp[r][k];
        }
        w.loss[((size_t)blockIdx.x * 2 + s) * 4 + k] = sum;
    }
}

// out6 = g_loss, d_loss, mean(real logit), mean(fake logit), d_loss' real term, its fake term
__global__ __launch_bounds__(64) void pd_fwd_tail(int N, int T, const double* __restrict__ loss, float* __restrict__ out6) {
    __shared__ double tot[6];
    const int c = threadIdx.x;
    if (c < 6) {
        const int s = c / 3, k = c - 3 * s;
        double sum = 0.0;
        for (int i = 0; i < T; ++i) sum += loss[((size_t)i * 2 + s) * 4 + k];
        tot[c] = sum / N;
    }
    __syncthreads();
    if (c == 0) {
        out6[0] = (float)(tot[0] + tot[3]);
        out6[1] = (float)(tot[1] + tot[4]);
        out6[2] = (float)tot[2];
        out6[3] = (float)tot[5];
        out6[4] = (float)tot[1];
        out6[5] = (float)tot[4];
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// Right-hand side q = 0: dlogit_g, for the input gradients (dxf stored or accumulated with a scale); q = 1: dlogit_d, for the parameter
// gradients (dxf_d stored, the intermediate gradients kept in the workspace).
template <int H> __global__ __launch_bounds__(H) void pd_bwd_a(In in, Par p, Tape<H> t, Ws<H> w, const float* __restrict__ dlg, const float* __restrict__ dld,
                                                               int want_in, int want_par, float* __restrict__ dxf, int lddxf, float xscale, int xacc,
                                                               float* __restrict__ dxf_d) {
    __shared__ __align__(16) float ds[RT][H + 4];
    __shared__ __align__(16) float xs[RT][H + 4];
    __shared__ double st[RT][2];
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6, N = in.N, M = 2 * N;
    for (int q = 0; q < 2; ++q) {
        if (!(q == 0 ? want_in : want_par)) continue;
        const float* dl = q == 0 ? dlg : dld;
        float da4[RT];
        {
            const float wc = p.wc[c], gp = p.gp[c];
            float dxh[RT], xr[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const int n = r0 + r;
                float dn = 0.f, xh = 0.f;
                if (n < M) {
                    xh = t.xhat4[(size_t)n * H + c];
                    dn = dl[n] * wc * leaky_d(t.h4[(size_t)n * H + c]);          // sign(h4) = sign of the pre-activation
                    if (q == 1) w.dn4[(size_t)n * H + c] = dn;
                }
                dxh[r] = dn * gp;
                xr[r] = xh;
            }
            __syncthreads();                                                 // the previous right-hand side is done with ds / xs
            ln_backward<H>(dxh, xr, t.rstd4, r0, M, c, lane, wv, ds, xs, st, q == 1 ? w.da4 : nullptr, da4);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RT; ++r) ds[r][c] = da4[r];
        __syncthreads();
        double acc[RT];
        fc_t<H>(ds, p.wp, H + c, acc);                                       // d xf
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            if (n >= M) continue;
            if (q == 0) put(dxf + (size_t)n * lddxf + c, acc[r], xscale, xacc);
            else if (dxf_d) dxf_d[(size_t)n * H + c] = (float)acc[r];
        }
        fc_t<H>(ds, p.wp, c, acc);                                           // d zf
        float da3[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            da3[r] = 0.f;
            if (n < M) {
                da3[r] = (float)acc[r] * leaky_d(t.a3[(size_t)n * H + c]);
                if (q == 1) w.da3[(size_t)n * H + c] = da3[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RT; ++r) ds[r][c] = da3[r];
        __syncthreads();
        fc_t<H>(ds, p.w3, c, acc);                                           // d h2
        const double g2 = p.g2[c], be2 = p.be2[c];
        double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            if (n < M) {
                const int s = n >= N;
                const double xh = ((double)t.a2[(size_t)n * H + c] - t.bn[(2 * s) * H + c]) * t.bn[(2 * s + 1) * H + c];
                const float dn = (float)acc[r] * (float)leaky_d(fma(g2, xh, be2));
                w.dn2[((size_t)q * M + n) * H + c] = dn;
                s1[s] += (double)dn;
                s2[s] = fma((double)dn, xh, s2[s]);
            }
        }
        for (int s = 0; s < 2; ++s) { w.col(q, blockIdx.x, s, 0)[c] = s1[s]; w.col(q, blockIdx.x, s, 1)[c] = s2[s]; }
    }
}

template <int H> __global__ __launch_bounds__(H) void pd_bwd_b(In in, Par p, Tape<H> t, Ws<H> w, int training, int want_in, int want_par,
                                                               float* __restrict__ de, int ldde, float xscale, int xacc) {
    __shared__ __align__(16) float ds[RT][H + 4];
    __shared__ __align__(16) float xs[RT][H + 4];
    __shared__ double st[RT][2];
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6, N = in.N, M = 2 * N, L = in.L;
    for (int q = 0; q < 2; ++q) {
        if (!(q == 0 ? want_in : want_par)) continue;
        if (q == 0 && (!de || r0 >= N)) continue;                            // the input side ends in d e: segment 0's rows alone
        double mdn[2] = {0.0, 0.0}, mdx[2] = {0.0, 0.0};
        if (training) {
            for (int i = 0; i < w.T; ++i)
                for (int s = 0; s < 2; ++s) { mdn[s] += w.col(q, i, s, 0)[c]; mdx[s] += w.col(q, i, s, 1)[c]; }
            for (int s = 0; s < 2; ++s) { mdn[s] /= N; mdx[s] /= N; }
        }
        __syncthreads();                                                     // the previous right-hand side is done with ds / xs
        {
            const double g2 = p.g2[c];
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const int n = r0 + r;
                float v = 0.f;
                if (n < M) {
                    const int s = n >= N;
                    const double rs = t.bn[(2 * s + 1) * H + c], xh = ((double)t.a2[(size_t)n * H + c] - t.bn[(2 * s) * H + c]) * rs;
                    const double dn = w.dn2[((size_t)q * M + n) * H + c];
                    v = (float)(training ? g2 * rs * ((dn - mdn[s]) - xh * mdx[s]) : g2 * rs * dn);
                    if (q == 1) w.da2[(size_t)n * H + c] = v;
                }
                ds[r][c] = v;
            }
        }
        __syncthreads();
        double acc[RT];
        fc_t<H>(ds, p.w2, c, acc);                                           // d h1
        float da1[RT];
        {
            const float g1 = p.g1[c];
            float dxh[RT], xr[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const int n = r0 + r;
                float dn = 0.f, xh = 0.f;
                if (n < M) {
                    xh = t.xhat1[(size_t)n * H + c];
                    dn = (float)acc[r] * leaky_d(t.h1[(size_t)n * H + c]);
                    if (q == 1) w.dn1[(size_t)n * H + c] = dn;
                }
                dxh[r] = dn * g1;
                xr[r] = xh;
            }
            __syncthreads();                                                 // every thread is done reading ds in fc_t
            ln_backward<H>(dxh, xr, t.rstd1, r0, M, c, lane, wv, ds, xs, st, q == 1 ? w.da1 : nullptr, da1);
        }
        if (q == 1) continue;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RT; ++r) ds[r][c] = da1[r];
        __syncthreads();
        for (int o = c; o < RT * L; o += H) {
            const int r = o / L, j = o - r * L, n = r0 + r;
            if (n >= N) continue;
            double sum = 0.0;
            for (int k = 0; k < H; k += 4) {
                const float4 wv4 = *reinterpret_cast<const float4*>(&p.w1[(size_t)j * H + k]);
                const float4 d = *reinterpret_cast<const float4*>(&ds[r][k]);
                sum = fma((double)d.w, (double)wv4.w, fma((double)d.z, (double)wv4.z, fma((double)d.y, (double)wv4.y, fma((double)d.x, (double)wv4.x, sum))));
            }
            put(de + (size_t)n * ldde + j, sum, xscale, xacc);
        }
    }
}

// Parameter gradients from the workspace of right-hand side 1.  Thread = output column c; every sum walks the 2N rows upward.
// Workgroups: [0, 2H/KT) d Wp rows | H/KT of d W3 | H/KT of d W2 | ceil(L/KT) of d W1 | three of vectors.
template <int H> __global__ __launch_bounds__(H) void pd_bwd_params(In in, Par p, Tape<H> t, Ws<H> w, const float* __restrict__ dld, Grad g, float ps, int pacc) {
    constexpr int NBP = 2 * H / KT, NB = H / KT;
    const int c = threadIdx.x, N = in.N, M = 2 * N, L = in.L, nbj = (L + KT - 1) / KT;
    int b = blockIdx.x;
    double acc[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) acc[i] = 0.0;
    if (b < NBP) {
        const int k0 = b * KT;
        for (int n = 0; n < M; ++n) {
            const double d = w.da4[(size_t)n * H + c];
#pragma unroll
            for (int i = 0; i < KT; ++i) {
                const float v = k0 < H ? leaky(t.a3[(size_t)n * H + k0 + i]) : in.xf[(size_t)n * in.ldf + (k0 - H) + i];
                acc[i] = fma((double)v, d, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < KT; ++i) put(g.wp + (size_t)(k0 + i) * H + c, acc[i], ps, pacc);
        return;
    }
    b -= NBP;
    if (b < NB) {
        const int k0 = b * KT;
        double g2[KT], be2[KT];
#pragma unroll
        for (int i = 0; i < KT; ++i) { g2[i] = p.g2[k0 + i]; be2[i] = p.be2[k0 + i]; }
        for (int n = 0; n < M; ++n) {
            const int s = n >= N;
            const double d = w.da3[(size_t)n * H + c];
#pragma unroll
            for (int i = 0; i < KT; ++i) {
                const double xh = ((double)t.a2[(size_t)n * H + k0 + i] - t.bn[(2 * s) * H + k0 + i]) * t.bn[(2 * s + 1) * H + k0 + i];
                acc[i] = fma((double)(float)leaky(fma(g2[i], xh, be2[i])), d, acc[i]);      // h2 as the forward rounded it
            }
        }
#pragma unroll
        for (int i = 0; i < KT; ++i) put(g.w3 + (size_t)(k0 + i) * H + c, acc[i], ps, pacc);
        return;
    }
    b -= NB;
    if (b < NB) {
        const int k0 = b * KT;
        for (int n = 0; n < M; ++n) {
            const double d = w.da2[(size_t)n * H + c];
            const float* hrow = t.h1 + (size_t)n * H + k0;
#pragma unroll
            for (int i = 0; i < KT; ++i) acc[i] = fma((double)hrow[i], d, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < KT; ++i) put(g.w2 + (size_t)(k0 + i) * H + c, acc[i], ps, pacc);
        return;
    }
    b -= NB;
    if (b < nbj) {
        const int j0 = b * KT;
        for (int n = 0; n < M; ++n) {
            const double d = w.da1[(size_t)n * H + c];
#pragma unroll
            for (int i = 0; i < KT; ++i)
                if (j0 + i < L) acc[i] = fma((double)load_code(in, n, j0 + i), d, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < KT; ++i)
            if (j0 + i < L) put(g.w1 + (size_t)(j0 + i) * H + c, acc[i], ps, pacc);
        return;
    }
    b -= nbj;
    if (b == 0) {                                                            // dis_pair's vectors
        for (int n = 0; n < M; ++n) {
            const double dn = w.dn4[(size_t)n * H + c], dl = dld[n];
            acc[0] += w.da4[(size_t)n * H + c];
            acc[1] = fma(dn, (double)t.xhat4[(size_t)n * H + c], acc[1]);
            acc[2] += dn;
            acc[3] = fma(dl, (double)t.h4[(size_t)n * H + c], acc[3]);
            acc[4] += dl;
        }
        put(g.bp + c, acc[0], ps, pacc);
        put(g.gp + c, acc[1], ps, pacc);
        put(g.bep + c, acc[2], ps, pacc);
        put(g.wc + c, acc[3], ps, pacc);
        if (c == 0) put(g.bc, acc[4], ps, pacc);
    } else if (b == 1) {                                                     // fc3's bias, BatchNorm's affine pair, fc2's bias
        for (int n = 0; n < M; ++n) {
            const int s = n >= N;
            const double xh = ((double)t.a2[(size_t)n * H + c] - t.bn[(2 * s) * H + c]) * t.bn[(2 * s + 1) * H + c];
            const double dn = w.dn2[((size_t)M + n) * H + c];
            acc[0] += w.da3[(size_t)n * H + c];
            acc[1] = fma(dn, xh, acc[1]);
            acc[2] += dn;
            acc[3] += w.da2[(size_t)n * H + c];
        }
        put(g.b3 + c, acc[0], ps, pacc);
        put(g.g2 + c, acc[1], ps, pacc);
        put(g.be2 + c, acc[2], ps, pacc);
        put(g.b2 + c, acc[3], ps, pacc);
    } else {                                                                 // LayerNorm-1's affine pair, fc1's bias
        for (int n = 0; n < M; ++n) {
            const double dn = w.dn1[(size_t)n * H + c];
            acc[0] = fma(dn, (double)t.xhat1[(size_t)n * H + c], acc[0]);
            acc[1] += dn;
            acc[2] += w.da1[(size_t)n * H + c];
        }
        put(g.g1 + c, acc[0], ps, pacc);
        put(g.be1 + c, acc[1], ps, pacc);
        put(g.b1 + c, acc[2], ps, pacc);
    }
}

constexpr int HB = 128;                                                      // the one width that is built (and tested)

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_pair_disc_supported(int N, int L, int Hd, int training) {
    if (Hd != HB) return mi_set_error(0, "mi_pair_disc: hidden width %d (only 128 is built)", Hd), 0;
    if (L < 1 || L > LMAX) return mi_set_error(0, "mi_pair_disc: code width %d outside [1, 128]", L), 0;
    if (N < (training ? 2 : 1) || N > MI_PAIR_DISC_NMAX)
        return mi_set_error(0, "mi_pair_disc: %d rows per segment outside [%d, %d] (BatchNorm1d needs 2 in training)", N, training ? 2 : 1, MI_PAIR_DISC_NMAX), 0;
    return 1;
}

extern "C" size_t mi_pair_disc_tape_floats(int N, int Hd) { return (N > 0 && Hd == HB) ? tape_floats<HB>(2 * N) : 0; }
extern "C" size_t mi_pair_disc_workspace_floats(int N, int Hd) { return (N > 0 && Hd == HB) ? ws_floats<HB>(2 * N) : 0; }

static int pd_input(int N, int L, const float* e, int lde, const float* z, int ldz, const float* xf, int ldf, In* in) {
    if (!e || !z || !xf || lde < L || ldz < L || ldf < HB) return -1;
    *in = In{N, L, e, lde, z, ldz, xf, ldf};
    return 0;
}
template <class P> static bool all_sixteen(P* const* q, bool aligned) {
    for (int i = 0; i < 16; ++i)
        if (!q[i] || (aligned && !aligned16(q[i]))) return false;
    return true;
}

extern "C" int mi_pair_disc_fwd(int N, int L, int Hd, const float* e, int lde, const float* z, int ldz, const float* xf, int ldf,
                                const float* const* params, int training, int loss_mode, float momentum, float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, float* tape, float* workspace, float* logit, float* dlogit_g, float* dlogit_d,
                                float* out6, void* stream) {
    MI_REQUIRE(mi_pair_disc_supported(N, L, Hd, training) == 1, "shape not supported (H == 128, 1 <= L <= 128, N >= 2 per segment in training)");
    MI_REQUIRE(params && tape && workspace && logit && dlogit_g && dlogit_d && out6, "bad argument");
    In in;
    MI_REQUIRE(pd_input(N, L, e, lde, z, ldz, xf, ldf, &in) == 0, "inputs: e (lde >= L), z (ldz >= L), xf (ldf >= H)");
    MI_REQUIRE(all_sixteen(params, true), "parameters: sixteen 16-byte-aligned pointers");
    MI_REQUIRE(loss_mode >= 0 && loss_mode <= 2, "loss_mode: 0 vanilla, 1 lsgan, 2 hinge");
    MI_REQUIRE(training || (running_mean && running_var), "evaluation mode needs the running statistics");
    MI_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
    MI_REQUIRE(aligned16(tape) && aligned16(workspace), "tape, workspace: 16-byte alignment");
    const Par p = par_of(params);
    const int M = 2 * N, T = (M + RT - 1) / RT;
    Tape<HB> t(tape, M);
    Ws<HB> w(workspace, M);
    hipLaunchKernelGGL(pd_fwd_a<HB>, dim3(T), dim3(HB), 0, ST, in, p, t, w);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(pd_fwd_b<HB>, dim3(T), dim3(HB), 0, ST, in, p, t, w, training ? 1 : 0, loss_mode, momentum, running_mean, running_var,
                       training ? num_batches_tracked : nullptr, logit, dlogit_g, dlogit_d);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(pd_fwd_tail, dim3(1), dim3(64), 0, ST, N, T, w.loss, out6);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_pair_disc_bwd(int N, int L, int Hd, const float* e, int lde, const float* z, int ldz, const float* xf, int ldf,
                                const float* const* params, int training, const float* tape, float* workspace, const float* dlogit_g,
                                const float* dlogit_d, float* dxf, int lddxf, float* de, int ldde, float in_scale, int accumulate_in,
                                float* const* grads, float* dxf_d, float param_scale, int accumulate_params, void* stream) {
    MI_REQUIRE(mi_pair_disc_supported(N, L, Hd, training) == 1, "shape not supported (H == 128, 1 <= L <= 128, N >= 2 per segment in training)");
    MI_REQUIRE(params && tape && workspace, "bad argument");
    const int want_in = dxf != nullptr, want_par = grads != nullptr;
    MI_REQUIRE(want_in || want_par, "neither input gradients (dxf) nor parameter gradients (grads) asked for");
    MI_REQUIRE(want_in || !de, "de comes with dxf");
    MI_REQUIRE(!want_in || (dlogit_g && lddxf >= HB && (!de || ldde >= L)), "input gradients: dlogit_g, lddxf >= H, ldde >= L");
    MI_REQUIRE(!want_par || (dlogit_d && all_sixteen(grads, false)), "parameter gradients: dlogit_d and sixteen gradient pointers");
    In in;
    MI_REQUIRE(pd_input(N, L, e, lde, z, ldz, xf, ldf, &in) == 0, "inputs: e (lde >= L), z (ldz >= L), xf (ldf >= H)");
    MI_REQUIRE(all_sixteen(params, true), "parameters: sixteen 16-byte-aligned pointers");
    MI_REQUIRE(aligned16(tape) && aligned16(workspace), "tape, workspace: 16-byte alignment");
    const Par p = par_of(params);
    const Grad g = grad_of(grads);
    const int M = 2 * N, T = (M + RT - 1) / RT;
    Tape<HB> t(const_cast<float*>(tape), M);
    Ws<HB> w(workspace, M);
    hipLaunchKernelGGL(pd_bwd_a<HB>, dim3(T), dim3(HB), 0, ST, in, p, t, w, dlogit_g, dlogit_d, want_in, want_par, dxf, lddxf, in_scale,
                       accumulate_in ? 1 : 0, dxf_d);
    MI_LAUNCH_CHECK();
    if (want_par || de) {
        hipLaunchKernelGGL(pd_bwd_b<HB>, dim3(T), dim3(HB), 0, ST, in, p, t, w, training ? 1 : 0, want_in, want_par, de, ldde, in_scale,
                           accumulate_in ? 1 : 0);
        MI_LAUNCH_CHECK();
    }
    if (want_par) {
        hipLaunchKernelGGL(pd_bwd_params<HB>, dim3(2 * HB / KT + 2 * (HB / KT) + (L + KT - 1) / KT + 3), dim3(HB), 0, ST, in, p, t, w, dlogit_d, g,
                           param_scale, accumulate_params ? 1 : 0);
        MI_LAUNCH_CHECK();
    }
    return 0;
}
