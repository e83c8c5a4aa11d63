// Operators of the VAE-GAN (reference src/models/vae_gan.py:63-102) that the VAE and GAN paths do not have.  All of them are streaming
// and memory-bound; rows have pitches that are multiples of 4 floats and every store is one 16-byte access per lane:
//   * the latent block that writes the decoder's 2N-row input [mu + exp(log_sigma) eps | prior] in one launch, with the KL term, and
//     its backward, which reads the recon half of the decoder's input gradient, undoes the recon_weight it carries and adds the KL
//     gradient;
//   * the discriminator-feature reconstruction loss sum (real - recon)^2 / N on two segments of netD's last hidden NHWC activation,
//     read in place, with the gradient by the recon segment stored or added into netD's gradient buffer;
//   * the segment packing [fake | nhwc(imgs) | recon] of netD's input, and the decoder's upstream gradient
//     [s_recon dX_recon | s_fake dX_fake] out of netD's input gradient: one launch each way.
// fp32 tensors, every sum fp64 in a fixed order and rounded once, no atomics, every element of every output stored (pad lanes as 0),
// the workspace needs no zeroing: two runs agree bit for bit.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TPB = 256;
constexpr int FM_WG = 1024;                                        // feature-match partial sums: at most this many workgroups

inline int nblk(size_t n) { size_t b = (n + TPB - 1) / TPB; return (int)(b > 4096 ? 4096 : (b ? b : 1)); }

// Workgroups [0, gridDim.x - 1): one thread per 4-lane group of z [2N][ldz].  Rows [0, N) = mu + exp(log_sigma) eps, rows [N, 2N) =
// prior, lanes from L on 0.  The last workgroup alone forms the KL term (mi_vae_latent_fwd's formula per element, summed in fp64 in a
// fixed order) and stores it.
__global__ __launch_bounds__(TPB) void vaegan_latent_fwd_kernel(int N, int L, const float* __restrict__ h, int ldh,
                                                                const float* __restrict__ eps, const float* __restrict__ prior,
                                                                float* __restrict__ z, int ldz, float* __restrict__ kld) {
    __shared__ double red[4];
    if (blockIdx.x == gridDim.x - 1) {
        const int total = N * L;
        double acc = 0.0;
        for (int i = threadIdx.x; i < total; i += TPB) {
            const int n = i / L, k = i - n * L;
            const float mu = h[(size_t)n * ldh + k], ls = h[(size_t)n * ldh + L + k];
            const float sg = expf(ls);
            acc += (double)(-0.5f * (1.f + 2.f * ls - mu * mu - sg * sg));
        }
        acc = block_sum_256d(acc, red);
        if (threadIdx.x == 0) *kld = (float)(acc / (double)N);
        return;
    }
    const int Q = ldz / 4, nb = gridDim.x - 1;
    const int total = 2 * N * Q;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < total; i += nb * TPB) {
        const int r = i / Q, q = i - r * Q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * q + j;
            if (k < L) {
                if (r < N) v[j] = h[(size_t)r * ldh + k] + expf(h[(size_t)r * ldh + L + k]) * eps[(size_t)r * L + k];
                else v[j] = prior[(size_t)(r - N) * L + k];
            }
        }
        *reinterpret_cast<f32x4*>(z + (size_t)r * ldz + 4 * q) = v;
    }
}

// One thread per 4-lane group of dh [N][lddh]: lanes [0, L) = d + gk mu, [L, 2L) = d eps exp(ls) + gk (exp(2 ls) - 1), the rest 0;
// d = dz_scale * dz[n][k], gk = g_kld / N.
__global__ __launch_bounds__(TPB) void vaegan_latent_bwd_kernel(int N, int L, const float* __restrict__ h, int ldh,
                                                                const float* __restrict__ eps, const float* __restrict__ dz, int lddz,
                                                                float dz_scale, float g_kld, float* __restrict__ dh, int lddh) {
    const int Q = lddh / 4, total = N * Q;
    const float gk = g_kld / (float)N;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < total; i += gridDim.x * TPB) {
        const int n = i / Q, q = i - n * Q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * q + j;
            if (c < 2 * L) {
                const int k = c < L ? c : c - L;
                const float mu = h[(size_t)n * ldh + k], ls = h[(size_t)n * ldh + L + k];
                const float sg = expf(ls), d = dz_scale * dz[(size_t)n * lddz + k];
                v[j] = c < L ? d + gk * mu : d * eps[(size_t)n * L + k] * sg + gk * (sg * sg - 1.f);
            }
        }
        *reinterpret_cast<f32x4*>(dh + (size_t)n * lddh + 4 * q) = v;
    }
}

// ws[workgroup] = sum over its 4-lane groups of (real - recon)^2 in fp64; drecon (nullable) = k (recon - real), stored or added.
__global__ __launch_bounds__(TPB) void feat_match_rows(size_t n4, const f32x4* __restrict__ real, const f32x4* __restrict__ recon,
                                                       f32x4* drecon, double k, int accumulate, double* __restrict__ ws) {
    __shared__ double red[4];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += (size_t)gridDim.x * TPB) {
        const f32x4 a = real[i], b = recon[i];
        f32x4 g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = (double)b[j] - (double)a[j];
            acc = fma(d, d, acc);
            g[j] = (float)(k * d);
        }
        if (drecon) drecon[i] = accumulate ? drecon[i] + g : g;
    }
    acc = block_sum_256d(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

__global__ __launch_bounds__(TPB) void feat_match_reduce(int nws, double inv, const double* __restrict__ ws, float* __restrict__ loss) {
    __shared__ double red[4];
    double v = 0.0;
    for (int i = threadIdx.x; i < nws; i += TPB) v += ws[i];
    v = block_sum_256d(v, red);
    if (threadIdx.x == 0) loss[0] = (float)(v * inv);
}

inline int fm_grid(int N, int per) {
    const size_t n4 = (size_t)N * per / 4, n = (n4 + TPB - 1) / TPB;
    return (int)(n < (size_t)FM_WG ? n : (size_t)FM_WG);
}

// dst [S * N][HW][ld]: segment s is a scaled copy of src_s (NHWC [N][HW][ld], or NCHW [N][C][HW] when nchw is set); lanes from C on 0.
struct SegSrc { const float* p; float scale; int nchw; };

__global__ __launch_bounds__(TPB) void seg_gather_kernel(int S, int N, int C, int HW, int ld, SegSrc s0, SegSrc s1, SegSrc s2,
                                                         float* __restrict__ dst) {
    const int Q = ld / 4;
    const size_t per = (size_t)N * HW * Q, total = per * S;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const int s = (int)(i / per);
        const size_t e = i - (size_t)s * per;                     // (pixel of the segment, 4-lane group)
        const SegSrc src = s == 0 ? s0 : (s == 1 ? s1 : s2);
        const int q = (int)(e % Q);
        const size_t px = e / Q;
        f32x4 v;
        if (src.nchw) {
            const size_t n = px / HW, p = px - n * HW;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = 4 * q + j < C ? src.p[(n * C + 4 * q + j) * HW + p] : 0.f;
        } else {
            v = *reinterpret_cast<const f32x4*>(src.p + e * 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 4 * q + j < C ? v[j] * src.scale : 0.f;
        *reinterpret_cast<f32x4*>(dst + i * 4) = v;
    }
}

bool pack_ok(const char* fn, int N, int C, int HW, int ld) {
    if (N < 1 || C < 1 || HW < 1 || ld < C || ld % 4 != 0)
        return mi_set_error(0, "%s: N, C, HW >= 1 and a pixel pitch ld >= C that is a multiple of 4 (got N=%d C=%d HW=%d ld=%d)", fn, N, C, HW, ld), false;
    if ((long long)3 * N * HW * ld >= (1ll << 31)) return mi_set_error(0, "%s: 3 N HW ld below 2^31", fn), false;
    return true;
}

}  // namespace

#define ST ((hipStream_t)stream)
#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

extern "C" int mi_vaegan_latent_supported(int N, int L) {
    if (N < 1 || L < 1 || (long long)N * (L + 3) >= (1ll << 27))
        return mi_set_error(0, "mi_vaegan_latent: N >= 1, L >= 1 and N (L + 3) below 2^27 (got N=%d L=%d)", N, L), 0;
    return 1;
}

extern "C" int mi_vaegan_latent_fwd(int N, int L, const float* h, int ldh, const float* eps, const float* prior, float* z, int ldz,
                                    float* kld, void* stream) {
    if (!mi_vaegan_latent_supported(N, L)) return -1;                     // the message is set
    MI_REQUIRE(h && eps && prior && z && kld, "null pointer");
    MI_REQUIRE(ldh >= 2 * L, "ldh < 2 L");
    MI_REQUIRE(ldz == (L + 3) / 4 * 4 && AL16(z), "ldz = 4 ceil(L / 4) and a 16-byte aligned z are expected");
    hipLaunchKernelGGL(vaegan_latent_fwd_kernel, dim3(nblk((size_t)2 * N * (ldz / 4)) + 1), dim3(TPB), 0, ST, N, L, h, ldh, eps, prior, z, ldz,
                       kld);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_vaegan_latent_bwd(int N, int L, const float* h, int ldh, const float* eps, const float* dz, int lddz, float dz_scale,
                                    float g_kld, float* dh, int lddh, void* stream) {
    if (!mi_vaegan_latent_supported(N, L)) return -1;
    MI_REQUIRE(h && eps && dz && dh, "null pointer");
    MI_REQUIRE(ldh >= 2 * L && lddz >= L, "ldh < 2 L or lddz < L");
    MI_REQUIRE(lddh >= 2 * L && lddh % 4 == 0 && lddh <= 2 * L + 3 && AL16(dh), "lddh = 4 ceil(2 L / 4) and a 16-byte aligned dh are expected");
    hipLaunchKernelGGL(vaegan_latent_bwd_kernel, dim3(nblk((size_t)N * (lddh / 4))), dim3(TPB), 0, ST, N, L, h, ldh, eps, dz, lddz, dz_scale,
                       g_kld, dh, lddh);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_feat_match_supported(int N, int per) {
    if (N < 1 || per < 4 || per % 4 != 0 || (long long)N * per >= (1ll << 31))
        return mi_set_error(0, "mi_feat_match: N >= 1, per a multiple of 4 and N per below 2^31 (got N=%d per=%d)", N, per), 0;
    return 1;
}

extern "C" size_t mi_feat_match_workspace_doubles(int N, int per) { return (N > 0 && per >= 4) ? (size_t)fm_grid(N, per) : 0; }

extern "C" int mi_feat_match(int N, int per, const float* real, const float* recon, float* loss, float* drecon, float gscale,
                             int accumulate, double* ws, void* stream) {
    if (!mi_feat_match_supported(N, per)) return -1;
    MI_REQUIRE(real && recon && loss && ws, "null pointer");
    MI_REQUIRE(AL16(real) && AL16(recon) && AL16(drecon), "16-byte aligned blocks are expected");
    const int grid = fm_grid(N, per);
    hipLaunchKernelGGL(feat_match_rows, dim3(grid), dim3(TPB), 0, ST, (size_t)N * per / 4, (const f32x4*)real, (const f32x4*)recon,
                       (f32x4*)drecon, 2.0 * (double)gscale / (double)N, accumulate, ws);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(feat_match_reduce, dim3(1), dim3(TPB), 0, ST, grid, 1.0 / (double)N, ws, loss);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_vaegan_pack_supported(int N, int C, int HW, int ld) { return pack_ok("mi_vaegan_pack", N, C, HW, ld) ? 1 : 0; }

extern "C" int mi_vaegan_pack_fwd(int N, int C, int HW, const float* dec_out, const float* imgs_nchw, float* x, int ld, void* stream) {
    if (!pack_ok(__func__, N, C, HW, ld)) return -1;
    MI_REQUIRE(dec_out && imgs_nchw && x && AL16(dec_out) && AL16(x), "null or misaligned pointer");
    const size_t seg = (size_t)N * HW * ld;
    const SegSrc fake = {dec_out + seg, 1.f, 0}, real = {imgs_nchw, 1.f, 1}, recon = {dec_out, 1.f, 0};
    hipLaunchKernelGGL(seg_gather_kernel, dim3(nblk(3 * seg / 4)), dim3(TPB), 0, ST, 3, N, C, HW, ld, fake, real, recon, x);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_vaegan_unpack_bwd(int N, int C, int HW, const float* dx, float s_recon, float s_fake, float* dy, int ld, void* stream) {
    if (!pack_ok(__func__, N, C, HW, ld)) return -1;
    MI_REQUIRE(dx && dy && AL16(dx) && AL16(dy), "null or misaligned pointer");
    const size_t seg = (size_t)N * HW * ld;
    const SegSrc recon = {dx + 2 * seg, s_recon, 0}, fake = {dx, s_fake, 0};
    hipLaunchKernelGGL(seg_gather_kernel, dim3(nblk(2 * seg / 4)), dim3(TPB), 0, ST, 2, N, C, HW, ld, recon, fake, fake, dy);
    MI_LAUNCH_CHECK();
    return 0;
}
