// The AGE's latent-moment operators (reference src/models/age.py:64-81, 90-92, 97-116, 129-144): everything between the encoder's
// output and the scalar losses, and back.
//   e [S*M, L] (the encoder's NHWC output, read in place with a pitch; S <= 2 segments of M rows)
//   z      = e / max(||e||_2, 1e-12) per row (F.normalize), or z = e without normalisation
//   mu_j   = mean_i z_ij, var_j = sum_i (z_ij - mu_j)^2 / (M - 1) per segment (torch's unbiased var)
//   kl     = mean_j (mu_j^2 + var_j - log var_j) / 2
//   recon  = 1 - mean_i cos(z_i, t_i) (mode 1, torch's cosine_similarity with eps = 1e-8) or mean_ij (z_ij - t_ij)^2 (mode 2)
//   forward   rows  : one wave per row: the norm, z, the row's reconstruction term              (skipped when there is nothing for it to do)
//             stats : one workgroup per segment: mu, var, kl, mean(mu), mean(var), the reconstruction loss
//   backward  rows  : one wave per row: g = c_s dkl/dz + w_s drecon/dz + dz_ext, then through the normalisation
//   image MSE rows + reduce: the recon_x term (age.py:109, 142) with its gradient, summed in a fixed order
// Conventions as csrc/info_head.hip: every tensor fp32, every sum fp64 in a fixed order and rounded once, no atomics, every element of
// every output stored, the workspace needs no zeroing.  Row n is computed by the same instruction sequence whichever workgroup it
// falls into.  Loads are scalar and coalesced along the row: no pitch or base alignment is assumed.
#include "common.h"

namespace {

constexpr int LMAX = 512, PER = LMAX / 64, RPB = 4, TPB = 256;
constexpr double NORM_EPS = 1e-12, COS_EPS = 1e-8;

// The row's cosine pieces from a (the code row) and t (the target row), both in registers, lane l holding columns l, l + 64, ...:
// na = ||a||, nt = ||t||, dot = a . t.  torch divides each row by its norm clamped at eps and sums the products.
__device__ __forceinline__ void cos_parts(const double* a, const double* t, double& na, double& nt, double& dot) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < PER; ++i) { s0 = fma(a[i], a[i], s0); s1 = fma(t[i], t[i], s1); s2 = fma(a[i], t[i], s2); }
    na = sqrt(wave_sum_d(s0));
    nt = sqrt(wave_sum_d(s1));
    dot = wave_sum_d(s2);
}

// ------------------------------------------------------------------------------------------------------------------ forward
// z [rows][L] dense and norm [rows] are stored when normalize is set; ws[n] = the row's reconstruction term (cos or sum of squares)
// for the rows of a segment with a mode.
__global__ __launch_bounds__(TPB) void age_fwd_rows(int M, int rows, int L, const float* __restrict__ e, int ld, int normalize,
                                                    float* __restrict__ z, float* __restrict__ norm, int mode0, int mode1,
                                                    const float* __restrict__ t, int ldt, double* __restrict__ ws) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (n >= rows) return;                                                   // whole waves leave: no barrier follows
    const int s = n >= M ? 1 : 0, mode = s ? mode1 : mode0;
    double a[PER];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = lane + 64 * i;
        a[i] = j < L ? (double)e[(size_t)n * ld + j] : 0.0;
        ss = fma(a[i], a[i], ss);
    }
    if (normalize) {
        const double nr = sqrt(wave_sum_d(ss)), inv = 1.0 / fmax(nr, NORM_EPS);
        if (lane == 0) norm[n] = (float)nr;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = lane + 64 * i;
            const float v = (float)(a[i] * inv);
            if (j < L) z[(size_t)n * L + j] = v;
            a[i] = v;                                                        // the losses see what was stored
        }
    }
    if (mode == 0) return;
    double tv[PER];
    const int m = n - s * M;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = lane + 64 * i;
        tv[i] = j < L ? (double)t[(size_t)m * ldt + j] : 0.0;
    }
    double r;
    if (mode == 1) {
        double na, nt, dot;
        cos_parts(a, tv, na, nt, dot);
        r = dot / (fmax(na, COS_EPS) * fmax(nt, COS_EPS));
    } else {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) { const double d = a[i] - tv[i]; q = fma(d, d, q); }
        r = wave_sum_d(q);
    }
    if (lane == 0) ws[n] = r;
}

// One workgroup per segment.  P columns (a power of two) are in flight, 256 / P row groups each walk their rows upward; the groups'
// partial sums are added in group order.  Two passes per column: the mean, then the squared deviations from it.
// out4 [S][4] = kl, mean(mu), mean(var), the reconstruction loss (0 without a mode).
__global__ __launch_bounds__(TPB) void age_fwd_stats(int M, int L, const float* __restrict__ x, int ldx, int mode0, int mode1,
                                                     const double* __restrict__ ws, float* __restrict__ mu, float* __restrict__ var,
                                                     float* __restrict__ out4) {
    __shared__ double part[TPB];
    __shared__ double mean_s[TPB];
    __shared__ double red[4];
    const int c = threadIdx.x, s = blockIdx.x, mode = s ? mode1 : mode0;
    int P = 1;
    while (P < L && P < TPB) P <<= 1;
    const int G = TPB / P, p = c & (P - 1), g = c / P;
    const float* xs = x + (size_t)s * M * ldx;
    double kl = 0.0, sm = 0.0, sv = 0.0;
    for (int j0 = 0; j0 < L; j0 += P) {
        const int j = j0 + p;
        double acc = 0.0;
        if (j < L)
            for (int r = g; r < M; r += G) acc += (double)xs[(size_t)r * ldx + j];
        __syncthreads();
        part[c] = acc;
        __syncthreads();
        if (g == 0) {
            double m = 0.0;
            for (int k = 0; k < G; ++k) m += part[k * P + p];
            mean_s[p] = m / M;
        }
        __syncthreads();
        const double mean = mean_s[p];
        acc = 0.0;
        if (j < L)
            for (int r = g; r < M; r += G) { const double d = (double)xs[(size_t)r * ldx + j] - mean; acc = fma(d, d, acc); }
        part[c] = acc;
        __syncthreads();
        if (g == 0 && j < L) {
            double q = 0.0;
            for (int k = 0; k < G; ++k) q += part[k * P + p];
            const double v = q / (M - 1);
            mu[(size_t)s * L + j] = (float)mean;
            var[(size_t)s * L + j] = (float)v;
            kl += mean * mean + v - log(v);
            sm += mean;
            sv += v;
        }
    }
    kl = block_sum_256d(kl, red);
    sm = block_sum_256d(sm, red);
    sv = block_sum_256d(sv, red);
    double r = 0.0;
    if (mode != 0)
        for (int n = c; n < M; n += TPB) r += ws[(size_t)s * M + n];
    r = block_sum_256d(r, red);
    if (c == 0) {
        out4[s * 4 + 0] = (float)(kl / (2.0 * L));
        out4[s * 4 + 1] = (float)(sm / L);
        out4[s * 4 + 2] = (float)(sv / L);
        out4[s * 4 + 3] = mode == 1 ? (float)(1.0 - r / M) : mode == 2 ? (float)(r / ((double)M * L)) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
struct Seg { float c, w; int mode; const float* dz_ext; };

// z: what the forward stored (pitch ldz), or e itself without normalisation (norm null).  de [rows][ldde], columns from L on stored as 0.
__global__ __launch_bounds__(TPB) void age_bwd_rows(int M, int rows, int L, const float* __restrict__ z, int ldz,
                                                    const float* __restrict__ norm, const float* __restrict__ mu,
                                                    const float* __restrict__ var, Seg s0, Seg s1, const float* __restrict__ t, int ldt,
                                                    int ldx, float* __restrict__ de, int ldde) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (n >= rows) return;
    const int s = n >= M ? 1 : 0, m = n - s * M;
    const Seg sg = s ? s1 : s0;
    double a[PER], g[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = lane + 64 * i;
        a[i] = j < L ? (double)z[(size_t)n * ldz + j] : 0.0;
        g[i] = (j < L && sg.dz_ext) ? (double)sg.dz_ext[(size_t)m * ldx + j] : 0.0;
    }
    if (sg.c != 0.f) {
        const double k = (double)sg.c / L, im = 1.0 / M, im1 = 1.0 / (M - 1);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = lane + 64 * i;
            if (j < L) {
                const double mj = mu[(size_t)s * L + j], vj = var[(size_t)s * L + j];
                g[i] += k * (mj * im + (1.0 - 1.0 / vj) * (a[i] - mj) * im1);
            }
        }
    }
    if (sg.mode != 0) {
        double tv[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = lane + 64 * i;
            tv[i] = j < L ? (double)t[(size_t)m * ldt + j] : 0.0;
        }
        if (sg.mode == 1) {
            // cos = (a / na^) . (t / nt^) with n^ = max(n, eps); torch clamps the norms in place outside the graph, so the norm's own
            // derivative a / ||a|| (0 at a = 0) applies on both sides of the clamp
            double na, nt, dot;
            cos_parts(a, tv, na, nt, dot);
            const double nah = fmax(na, COS_EPS), nth = fmax(nt, COS_EPS), k = -(double)sg.w / M;
            const double c1 = 1.0 / (nah * nth), c2 = na > 0.0 ? dot / (nah * nah * nth * na) : 0.0;
#pragma unroll
            for (int i = 0; i < PER; ++i) g[i] += k * (tv[i] * c1 - a[i] * c2);
        } else {
            const double k = 2.0 * (double)sg.w / ((double)M * L);
#pragma unroll
            for (int i = 0; i < PER; ++i) g[i] += k * (a[i] - tv[i]);
        }
    }
    if (norm) {
        const double nr = norm[n];
        if (nr >= NORM_EPS) {                                                // uniform over the wave
            double zg = 0.0;
#pragma unroll
            for (int i = 0; i < PER; ++i) zg = fma(a[i], g[i], zg);
            zg = wave_sum_d(zg);
            const double inv = 1.0 / nr;
#pragma unroll
            for (int i = 0; i < PER; ++i) g[i] = (g[i] - a[i] * zg) * inv;
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) g[i] = g[i] / NORM_EPS;             // clamp_min passes nothing to the norm below eps
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = lane + 64 * i;
        if (j < L) de[(size_t)n * ldde + j] = (float)g[i];
    }
    for (int j = L + lane; j < ldde; j += 64) de[(size_t)n * ldde + j] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ image MSE
// recon_x = mean (pred - target)^2 with pred NHWC (pixel pitch ld) and target NCHW, and dpred = gscale * 2 (pred - target) / (B C HW),
// every element of dpred [B*HW][ld] stored (lanes from C on as 0).  mi_eps_loss adds its workgroups' sums with an atomic; here
// workgroup b walks pixels b * 256 + t, + grid * 256, ... upward and stores its fp64 block sum in ws[b], and one workgroup adds the
// ws upward: the same bits on every run.  The grid depends on the shape alone.
constexpr int MSE_WG = 256;

__global__ __launch_bounds__(TPB) void age_mse_rows(int B, int C, int HW, const float* __restrict__ pred, int ld,
                                                    const float* __restrict__ target, float* __restrict__ dpred, float gscale,
                                                    double* __restrict__ ws) {
    __shared__ double red[4];
    const size_t npix = (size_t)B * HW;
    const double k = 2.0 * (double)gscale / ((double)npix * C);
    double acc = 0.0;
    for (size_t px = (size_t)blockIdx.x * TPB + threadIdx.x; px < npix; px += (size_t)gridDim.x * TPB) {
        const size_t b = px / HW, p = px - b * HW;
        for (int c = 0; c < ld; ++c) {
            float dv = 0.f;
            if (c < C) {
                const double d = (double)pred[px * ld + c] - (double)target[(b * C + c) * HW + p];
                acc = fma(d, d, acc);
                dv = (float)(k * d);
            }
            if (dpred) dpred[px * ld + c] = dv;
        }
    }
    acc = block_sum_256d(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

__global__ __launch_bounds__(TPB) void age_mse_reduce(int nws, double inv, const double* __restrict__ ws, float* __restrict__ loss) {
    __shared__ double red[4];
    double v = 0.0;
    for (int i = threadIdx.x; i < nws; i += TPB) v += ws[i];
    v = block_sum_256d(v, red);
    if (threadIdx.x == 0) loss[0] = (float)(v * inv);
}

inline int mse_grid(int B, int HW) {
    const size_t npix = (size_t)B * HW, n = (npix + TPB - 1) / TPB;
    return (int)(n < (size_t)MSE_WG ? n : (size_t)MSE_WG);
}

bool shape_ok(int S, int M, int L, int mmin) {
    if (S < 1 || S > 2) return mi_set_error(0, "mi_age_moments: %d segments (1 or 2 are built)", S), false;
    if (L < 1 || L > LMAX) return mi_set_error(0, "mi_age_moments: code width %d (1 to 512)", L), false;
    if (M < mmin || (long long)S * M > (1 << 24))
        return mi_set_error(0, mmin > 1 ? "mi_age_moments: %d rows per segment (the unbiased variance needs at least 2; 2^24 rows at the most)"
                                        : "mi_age_moments: %d rows per segment (at least 1; 2^24 rows at the most)", M), false;
    return true;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_age_moments_supported(int S, int M, int L) { return shape_ok(S, M, L, 2) ? 1 : 0; }

extern "C" size_t mi_age_moments_workspace_doubles(int S, int M) { return (S > 0 && M > 0) ? (size_t)S * M : 0; }

extern "C" int mi_age_moments_fwd(int S, int M, int L, const float* e, int ld, int normalize, float* z, float* norm, int want_stats,
                                  int mode0, int mode1, const float* t, int ldt, float* mu, float* var, float* out4, double* ws,
                                  void* stream) {
    if (!shape_ok(S, M, L, want_stats ? 2 : 1)) return -1;                   // the message is set
    MI_REQUIRE(e && ld >= L, "null code pointer or ld < L");
    MI_REQUIRE(normalize ? (z && norm) : (!z && !norm), "z and norm go with normalize");
    MI_REQUIRE(mode0 >= 0 && mode0 <= 2 && mode1 >= 0 && mode1 <= 2 && (S == 2 || mode1 == 0), "reconstruction modes 0, 1, 2 (mode1 with S = 2)");
    const bool recon = mode0 != 0 || mode1 != 0;
    MI_REQUIRE(!recon || (want_stats && t && ldt >= L && ws), "a reconstruction term needs the statistics, t (ldt >= L) and ws");
    MI_REQUIRE(want_stats ? (mu && var && out4) : (!mu && !var && !out4), "mu, var and out4 go with the statistics");
    MI_REQUIRE(normalize || want_stats, "nothing asked for");
    const int rows = S * M;
    if (normalize || recon) {
        hipLaunchKernelGGL(age_fwd_rows, dim3((rows + RPB - 1) / RPB), dim3(TPB), 0, ST, M, rows, L, e, ld, normalize, z, norm, mode0, mode1,
                           t, ldt, ws);
        MI_LAUNCH_CHECK();
    }
    if (want_stats) {
        hipLaunchKernelGGL(age_fwd_stats, dim3(S), dim3(TPB), 0, ST, M, L, normalize ? z : e, normalize ? L : ld, mode0, mode1, ws, mu, var,
                           out4);
        MI_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t mi_age_image_mse_workspace_doubles(int B, int HW) { return (B > 0 && HW > 0) ? (size_t)mse_grid(B, HW) : 0; }

extern "C" int mi_age_image_mse(int B, int C, int HW, const float* pred, int ld, const float* target, float* loss, float* dpred,
                                float gscale, double* ws, void* stream) {
    MI_REQUIRE(B >= 1 && C >= 1 && HW >= 1 && ld >= C, "B, C, HW >= 1 and ld >= C");
    MI_REQUIRE((long long)B * HW * ld < (1ll << 31), "B * HW * ld below 2^31");
    MI_REQUIRE(pred && target && loss && ws, "null pointer");
    const int grid = mse_grid(B, HW);
    hipLaunchKernelGGL(age_mse_rows, dim3(grid), dim3(TPB), 0, ST, B, C, HW, pred, ld, target, dpred, gscale, ws);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(age_mse_reduce, dim3(1), dim3(TPB), 0, ST, grid, 1.0 / ((double)B * C * HW), ws, loss);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_age_moments_bwd(int S, int M, int L, const float* z, int ldz, const float* norm, const float* mu, const float* var,
                                  float c0, float c1, int mode0, int mode1, float w0, float w1, const float* t, int ldt,
                                  const float* dz_ext0, const float* dz_ext1, int ldx, float* de, int ldde, void* stream) {
    if (!shape_ok(S, M, L, 2)) return -1;
    MI_REQUIRE(z && ldz >= L && de && ldde >= L, "null pointer, ldz < L or ldde < L");
    MI_REQUIRE(mode0 >= 0 && mode0 <= 2 && mode1 >= 0 && mode1 <= 2, "reconstruction modes 0, 1, 2");
    MI_REQUIRE(S == 2 || (c1 == 0.f && mode1 == 0 && !dz_ext1), "one segment: c1 = 0, mode1 = 0, dz_ext1 null");
    MI_REQUIRE((c0 == 0.f && c1 == 0.f) || (mu && var), "a KL coefficient needs mu and var");
    MI_REQUIRE((mode0 == 0 && mode1 == 0) || (t && ldt >= L), "a reconstruction term needs t (ldt >= L)");
    MI_REQUIRE((!dz_ext0 && !dz_ext1) || ldx >= L, "dz_ext: ldx >= L");
    const int rows = S * M;
    const Seg s0 = {c0, w0, mode0, dz_ext0}, s1 = {c1, w1, mode1, dz_ext1};
    hipLaunchKernelGGL(age_bwd_rows, dim3((rows + RPB - 1) / RPB), dim3(TPB), 0, ST, M, rows, L, z, ldz, norm, mu, var, s0, s1, t, ldt, ldx,
                       de, ldde);
    MI_LAUNCH_CHECK();
    return 0;
}
