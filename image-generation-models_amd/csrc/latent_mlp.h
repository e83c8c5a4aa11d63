// Row-tile steps of the latent discriminators, MLPEncoder(L, [256, 256], 1) of reference src/networks/basic.py:64-112.
// csrc/latent_disc.hip (second norm BatchNorm1d, FactorVAE) and csrc/latent_disc_ln.hip (second norm LayerNorm, two segments, AAE) are
// this network up to the second norm and back down from it; what the two share is here, once.  A workgroup of TPB threads owns a tile
// of RT rows, thread c owns column c.  The helpers take plain pointers: the two tapes and workspaces are laid out differently.
// Conventions: weights input-major ([in][out]: thread = output column reads them coalesced), plain FMA, every tensor fp32, every SUM
// accumulated in fp64 in a fixed order and rounded once, no atomics: two runs on the same inputs agree bit for bit.
// A helper is told a row-element loader, the type T below, a row limit and whether to store, never which file called it: a step that
// differs between the two stays in its file.
#pragma once
#include "common.h"

namespace {

constexpr int H = 256, TPB = 256, RT = 8, LMAX = 64, LDP = H + 4;
constexpr int KT = 8, NB_W2 = H / KT;                                        // the parameter kernel: KT weight rows per workgroup
constexpr float SLOPE = 0.2f, EPS = 1e-5f;

struct Par { const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3; };
struct Grad { float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3; };

inline Par par_of(const float* const* q) { return Par{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]}; }
inline Grad grad_of(float* const* q) { return q ? Grad{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]} : Grad{}; }
template <class P> inline bool all_ten_set(P* const* q) {
    for (int i = 0; i < 10; ++i)
        if (!q[i]) return false;
    return true;
}
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }
__device__ __forceinline__ float leaky_d(float v) { return v > 0.f ? 1.f : SLOPE; }
__device__ __forceinline__ double leaky(double v) { return v > 0.0 ? v : (double)SLOPE * v; }
__device__ __forceinline__ double leaky_d(double v) { return v > 0.0 ? 1.0 : (double)SLOPE; }

__device__ __forceinline__ void put(float* p, double v, float scale, int accumulate) {
    *p = (float)(accumulate ? fma((double)scale, v, (double)*p) : (double)scale * v);
}

// xs[r][j] = load(r0 + r, j) for the rows of the tile below N, 0 for the others.  load(n, j) -> float is element j of row n.
template <class Load> __device__ __forceinline__ void stage_rows(float (*xs)[LMAX], int r0, int N, int L, Load load) {
    for (int i = threadIdx.x; i < RT * L; i += TPB) {
        const int r = i / L, j = i - r * L;
        xs[r][j] = (r0 + r < N) ? load(r0 + r, j) : 0.f;
    }
}

// acc[r] = b1[c] + sum_j xs[r][j] W1[j][c], j upward, rounded once; parked in hs[r][c] as well, for the statistics pass
__device__ __forceinline__ void fc_in(const float (*xs)[LMAX], const float* w1, const float* b1, int L, int c, float* acc, float (*hs)[LDP]) {
    double a[RT];
    const double b = b1[c];
#pragma unroll
    for (int r = 0; r < RT; ++r) a[r] = b;
    for (int j = 0; j < L; ++j) {
        const double w = w1[(size_t)j * H + c];
#pragma unroll
        for (int r = 0; r < RT; ++r) a[r] = fma((double)xs[r][j], w, a[r]);
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) { acc[r] = (float)a[r]; hs[r][c] = acc[r]; }
}

// acc[r] = bias + sum_k hs[r][k] W[k][c] for the RT rows in hs (W input-major), k upward
__device__ __forceinline__ void fc256(const float (*hs)[LDP], const float* __restrict__ w, double bias, int c, double* acc) {
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = bias;
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

// the transpose, for the backward: acc[r] = sum_k ds[r][k] W[c][k], along this thread's row of the [in][out] weights
__device__ __forceinline__ void fc256_t(const float (*ds)[LDP], const float* w, int c, double* acc) {
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = 0.0;
    for (int k = 0; k < H; k += 4) {
        const float4 wv4 = *reinterpret_cast<const float4*>(&w[(size_t)c * H + k]);
        const double w0 = wv4.x, w1 = wv4.y, w2 = wv4.z, w3 = wv4.w;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float4 d = *reinterpret_cast<const float4*>(&ds[r][k]);
            acc[r] = fma((double)d.w, w3, fma((double)d.z, w2, fma((double)d.y, w1, fma((double)d.x, w0, acc[r]))));
        }
    }
}

// LayerNorm over a row of H.  The sums are fp64; T is the type their two results are KEPT in and the normalisation continues in.
//   T = double (latent_disc_ln.hip) is the sounder form: rounding a row's mean to fp32 would shift all 256 of its elements the same way,
//     an error the sums downstream do not average out.
//   T = float (latent_disc.hip) rounds the mean and rstd, and the two means of the backward, to fp32: that is what that file shipped
//     with and what its golden records were made with, so it stays until a change that is allowed to move its results.
// st[r] = (mean, rstd) of the RT rows in hs: one wave per row, two passes.
template <class T> __device__ __forceinline__ void ln_stats(const float (*hs)[LDP], T (*st)[2], int lane, int wv) {
    for (int r = wv; r < RT; r += 4) {
        const float4 v = *reinterpret_cast<const float4*>(&hs[r][4 * lane]);
        const double m = wave_sum_d(((double)v.x + v.y) + ((double)v.z + v.w)) * (1.0 / H);
        const double a = v.x - m, b = v.y - m, d = v.z - m, e = v.w - m;
        const double q = wave_sum_d((a * a + b * b) + (d * d + e * e)) * (1.0 / H);
        if (lane == 0) { st[r][0] = (T)m; st[r][1] = (T)(1.0 / sqrt(q + (double)EPS)); }
    }
}
template <class T> __device__ __forceinline__ float ln_xhat(float a, const T* st) { return (float)(((T)a - st[0]) * st[1]); }

// the two row means LayerNorm's backward needs: st[r] = (mean(d), mean(d * x)) of the RT rows in ds / xs
template <class T> __device__ __forceinline__ void ln_bwd_stats(const float (*ds)[LDP], const float (*xs)[LDP], T (*st)[2], int lane, int wv) {
    for (int r = wv; r < RT; r += 4) {
        const float4 d = *reinterpret_cast<const float4*>(&ds[r][4 * lane]);
        const float4 x = *reinterpret_cast<const float4*>(&xs[r][4 * lane]);
        const double s1 = wave_sum_d(((double)d.x + d.y) + ((double)d.z + d.w));
        const double s2 = wave_sum_d(((double)d.x * x.x + (double)d.y * x.y) + ((double)d.z * x.z + (double)d.w * x.w));
        if (lane == 0) { st[r][0] = (T)(s1 * (1.0 / H)); st[r][1] = (T)(s2 * (1.0 / H)); }
    }
}
// LayerNorm backward of the tile, from dxh = d xhat and xr = xhat (both 0 for rows from N on; staged in ds / xs, which must be free) to
// out[r] = d of the norm's input with the row's rstd[n * ldr]; stored in keep [N][H] as well unless that is null.  out may be dxh.
template <class T> __device__ __forceinline__ void ln_backward(const float* dxh, const float* xr, const float* rstd, int ldr, int r0, int N, int c,
                                                               int lane, int wv, float (*ds)[LDP], float (*xs)[LDP], T (*st)[2], float* keep, float* out) {
#pragma unroll
    for (int r = 0; r < RT; ++r) { ds[r][c] = dxh[r]; xs[r][c] = xr[r]; }
    __syncthreads();
    ln_bwd_stats<T>(ds, xs, st, lane, wv);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int n = r0 + r;
        float v = 0.f;
        if (n < N) {
            v = (float)((T)rstd[(size_t)n * ldr] * (((T)dxh[r] - st[r][0]) - (T)xr[r] * st[r][1]));
            if (keep) keep[(size_t)n * H + c] = v;
        }
        out[r] = v;
    }
}

// LayerNorm-1 forward from acc = fc1's output and its statistics: xhat1 and h1 = LeakyReLU(g xhat1 + be) stored for the rows below N,
// h1 parked in hs for fc2.
template <class T> __device__ __forceinline__ void ln_act_store(const float* acc, const T (*st)[2], float g, float be, int r0, int N, int c,
                                                                float* xhat1, float* h1, float (*hs)[LDP]) {
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const float xh = ln_xhat<T>(acc[r], st[r]);
        const float hv = leaky(fmaf(g, xh, be));
        if (r0 + r < N) {
            xhat1[(size_t)(r0 + r) * H + c] = xh;
            h1[(size_t)(r0 + r) * H + c] = hv;
        }
        hs[r][c] = hv;
    }
}

// From a0 = fc256_t's result (d h1) through LeakyReLU' and LayerNorm-1 backwards to da1[RT] (0 for rows from N on).  The row's rstd1
// is rstd1[n * ldr].  dn1_out / da1_out [N][H]: what the parameter kernel reads; null when the caller keeps no workspace.
template <class T> __device__ __forceinline__ void ln1_backward(const double* a0, float g1, const float* xhat1, const float* h1, const float* rstd1,
                                                                int ldr, int r0, int N, int c, int lane, int wv, float (*ds)[LDP], float (*xs)[LDP],
                                                                T (*st)[2], float* dn1_out, float* da1_out, float* da1) {
    float dxh[RT], xr[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int n = r0 + r;
        float dn = 0.f, xh = 0.f;
        if (n < N) {
            xh = xhat1[(size_t)n * H + c];
            dn = (float)a0[r] * leaky_d(h1[(size_t)n * H + c]);               // sign(h1) = sign of the pre-activation
            if (dn1_out) dn1_out[(size_t)n * H + c] = dn;
        }
        dxh[r] = dn * g1;
        xr[r] = xh;
    }
    __syncthreads();                                                         // every thread is done reading ds in fc256_t
    ln_backward<T>(dxh, xr, rstd1, ldr, r0, N, c, lane, wv, ds, xs, st, da1_out, da1);
}

// dx[n][j] (pitch ldx) = scale * sum_k da1[n][k] W1[j][k] for the rows of the tile below nlim, stored or accumulated; da1 goes through ds.
__device__ __forceinline__ void input_grad(const float* da1, float (*ds)[LDP], const float* w1, int L, int r0, int nlim, int c, float* dx, int ldx,
                                           float scale, int accumulate) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) ds[r][c] = da1[r];
    __syncthreads();
    for (int o = c; o < RT * L; o += TPB) {
        const int r = o / L, j = o - r * L, n = r0 + r;
        if (n >= nlim) continue;
        double sum = 0.0;
        for (int k = 0; k < H; k += 4) {
            const float4 wv4 = *reinterpret_cast<const float4*>(&w1[(size_t)j * H + k]);
            const float4 d = *reinterpret_cast<const float4*>(&ds[r][k]);
            sum = fma((double)d.w, (double)wv4.w, fma((double)d.z, (double)wv4.z, fma((double)d.y, (double)wv4.y, fma((double)d.x, (double)wv4.x, sum))));
        }
        put(dx + (size_t)n * ldx + j, sum, scale, accumulate);
    }
}

// The parameter kernel's workgroups [0, 32): d W2[k0 .. k0+8)[c]; [32, 32 + ceil(L/8)): d W1[j0 .. j0+8)[c] with the input through
// load(n, j); the next one: d b2, d gamma1, d beta1, d b1.  Thread = output column c; every sum walks the rows upward.
// Returns whether workgroup b was one of these.  The d W1 workgroup's loads are serial and it is the last to finish; with the range
// test as an early return in front, not as the chain's last else, the two kernels measured 14 % and 38 % slower.
template <class Load> __device__ __forceinline__ bool params_common(int b, int N, int L, Load load, const float* h1, const float* xhat1,
                                                                    const float* da2, const float* dn1, const float* da1, const Grad& g, float ps,
                                                                    int pacc) {
    const int c = threadIdx.x, nbj = (L + KT - 1) / KT;
    double acc[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) acc[i] = 0.0;
    if (b < NB_W2) {
        const int k0 = b * KT;
        for (int n = 0; n < N; ++n) {
            const double d = da2[(size_t)n * H + c];
            const float* hrow = h1 + (size_t)n * H + k0;
#pragma unroll
            for (int i = 0; i < KT; ++i) acc[i] = fma((double)hrow[i], d, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < KT; ++i) put(g.w2 + (size_t)(k0 + i) * H + c, acc[i], ps, pacc);
    } else if (b < NB_W2 + nbj) {
        const int j0 = (b - NB_W2) * KT;
        for (int n = 0; n < N; ++n) {
            const double d = da1[(size_t)n * H + c];
#pragma unroll
            for (int i = 0; i < KT; ++i)
                if (j0 + i < L) acc[i] = fma((double)load(n, j0 + i), d, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < KT; ++i)
            if (j0 + i < L) put(g.w1 + (size_t)(j0 + i) * H + c, acc[i], ps, pacc);
    } else if (b == NB_W2 + nbj) {
        for (int n = 0; n < N; ++n) {
            const double dn = dn1[(size_t)n * H + c];
            acc[0] += da2[(size_t)n * H + c];
            acc[1] = fma(dn, (double)xhat1[(size_t)n * H + c], acc[1]);
            acc[2] += dn;
            acc[3] += da1[(size_t)n * H + c];
        }
        put(g.b2 + c, acc[0], ps, pacc);
        put(g.g1 + c, acc[1], ps, pacc);
        put(g.be1 + c, acc[2], ps, pacc);
        put(g.b1 + c, acc[3], ps, pacc);
    } else {
        return false;
    }
    return true;
}

}  // namespace
