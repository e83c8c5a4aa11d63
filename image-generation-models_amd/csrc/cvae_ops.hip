// Operators of the label-conditioned VAE (reference src/models/cvae.py) that the VAE path does not have.  All three are label-indexed
// data movement the reference spells with one_hot().expand(), cat and nn.Embedding:
//   * the encoder input [image | one-hot label planes] written straight into the NHWC buffer the first conv reads (cvae.py:66-69),
//   * the decoder input [z | class_embedding(label)] produced by the latent block itself (cvae.py:44-46,72-73),
//   * the embedding table's gradient: a label-segmented sum of the decoder's input gradient.
// fp32, no atomics: every sum has a fixed order, so two runs on the same inputs agree bit for bit (graph replays rely on it).
// A label outside [0, ncls) selects nothing: no plane is set, the embedding half is zero, no gradient row is touched -- and nothing
// is ever indexed with it.
#include "common.h"

namespace {

constexpr int TPB = 256;

// y[n][p][c]: c < C image, C <= c < C + ncls one-hot plane of labels[n], c >= C + ncls zero.  Every element of y is stored.
__global__ __launch_bounds__(TPB) void cvae_pack_input_kernel(int N, int C, int HW, int ncls, const float* __restrict__ x,
                                                              const int64_t* __restrict__ labels, float* __restrict__ y, int ld) {
    const size_t tot = (size_t)N * HW * ld;
    for (size_t i = blockIdx.x * (size_t)TPB + threadIdx.x; i < tot; i += (size_t)gridDim.x * TPB) {
        const int c = (int)(i % ld);
        const size_t np = i / ld;
        const int p = (int)(np % HW), n = (int)(np / HW);
        float v = 0.f;
        if (c < C) v = x[((size_t)n * C + c) * HW + p];
        else if (c < C + ncls) v = labels[n] == (int64_t)(c - C) ? 1.f : 0.f;
        y[i] = v;
    }
}

// zc[n] = [mu + exp(log_sigma) eps | E[labels[n]]] over the first gridDim.x - 1 workgroups (h == nullptr: [eps | E[labels[n]]], the
// decode path).  The last workgroup alone forms the KL term, walking h in a fixed order, and stores it.
__global__ __launch_bounds__(TPB) void cvae_latent_fwd_kernel(int N, int L, int ncls, const float* __restrict__ h, int ldh,
                                                              const float* __restrict__ eps, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ E, float* __restrict__ zc, float* __restrict__ kld) {
    __shared__ float red[8];
    const int total = N * L;
    if (kld && blockIdx.x == gridDim.x - 1) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < total; i += TPB) {
            const int n = i / L, k = i - n * L;
            const float mu = h[(size_t)n * ldh + k], ls = h[(size_t)n * ldh + L + k];
            const float sg = expf(ls);
            acc += -0.5f * (1.f + 2.f * ls - mu * mu - sg * sg);
        }
        acc = block_sum_256(acc, red);
        if (threadIdx.x == 0) *kld = acc / (float)N;
        return;
    }
    const int nb = gridDim.x - (kld ? 1 : 0);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < 2 * total; i += nb * TPB) {
        const int n = i / (2 * L), k = i - n * 2 * L;
        float v;
        if (k < L) {
            v = eps[(size_t)n * L + k];
            if (h) v = h[(size_t)n * ldh + k] + expf(h[(size_t)n * ldh + L + k]) * v;
        } else {
            const int64_t c = labels[n];
            v = (c >= 0 && c < (int64_t)ncls) ? E[(size_t)c * L + (k - L)] : 0.f;
        }
        zc[i] = v;
    }
}

// Workgroups [0, nb_dh): dh = [dz + gk mu | dz eps exp(ls) + gk (exp(2 ls) - 1)], dz = dzc[:, :L], gk = g_kld (*g_dev) / N.
// Workgroups [nb_dh, ...): one thread per (class c, column j) walks the rows upward and adds the embedding halves of the rows
// labelled c; a class no row carries leaves its dE row alone.
__global__ __launch_bounds__(TPB) void cvae_latent_bwd_kernel(int N, int L, int ncls, const float* __restrict__ h, int ldh,
                                                              const float* __restrict__ eps, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ dzc, int lddzc, float g_kld,
                                                              const float* __restrict__ g_dev, float* __restrict__ dh,
                                                              float* __restrict__ dE, int nb_dh) {
    const int total = N * L;
    if ((int)blockIdx.x < nb_dh) {
        const float gk = g_kld * (g_dev ? g_dev[0] : 1.f) / (float)N;
        for (int i = blockIdx.x * TPB + threadIdx.x; i < total; i += nb_dh * TPB) {
            const int n = i / L, k = i - n * L;
            const float mu = h[(size_t)n * ldh + k], ls = h[(size_t)n * ldh + L + k];
            const float sg = expf(ls), d = dzc[(size_t)n * lddzc + k];
            dh[(size_t)n * 2 * L + k] = d + gk * mu;
            dh[(size_t)n * 2 * L + L + k] = d * eps[i] * sg + gk * (sg * sg - 1.f);
        }
        return;
    }
    const int i = ((int)blockIdx.x - nb_dh) * TPB + threadIdx.x;
    if (i >= ncls * L) return;
    const int c = i / L, j = i - c * L;
    float acc = 0.f;
    bool seen = false;
    for (int n = 0; n < N; ++n) {
        if (labels[n] == (int64_t)c) { acc += dzc[(size_t)n * lddzc + L + j]; seen = true; }
    }
    if (seen) dE[i] += acc;
}

inline int nblk(size_t n) { size_t b = (n + TPB - 1) / TPB; return (int)(b > 4096 ? 4096 : (b ? b : 1)); }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_cvae_pack_input(int N, int C, int HW, int ncls, const float* x_nchw, const int64_t* labels, float* y_nhwc, int ld,
                                  void* stream) {
    MI_REQUIRE(N > 0 && C > 0 && HW > 0 && ncls > 0 && x_nchw && labels && y_nhwc, "bad argument");
    MI_REQUIRE(ld >= C + ncls && (size_t)N * HW * ld < (1ull << 31), "ld < C + ncls, or more than 2^31 elements");
    hipLaunchKernelGGL(cvae_pack_input_kernel, dim3(nblk((size_t)N * HW * ld)), dim3(TPB), 0, ST, N, C, HW, ncls, x_nchw, labels, y_nhwc, ld);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_cvae_latent_fwd(int N, int L, int ncls, const float* h, int ldh, const float* eps, const int64_t* labels, const float* E,
                                  float* zc, float* kld, void* stream) {
    MI_REQUIRE(N > 0 && L > 0 && ncls > 0 && eps && labels && E && zc, "bad argument");
    MI_REQUIRE((size_t)N * L < (1ull << 29) && (size_t)ncls * L < (1ull << 31), "too many elements");
    MI_REQUIRE(h ? ldh >= 2 * L : kld == nullptr, "ldh < 2 L, or a KL term asked of the concatenate-only mode (h == null)");
    hipLaunchKernelGGL(cvae_latent_fwd_kernel, dim3(nblk((size_t)N * 2 * L) + (kld ? 1 : 0)), dim3(TPB), 0, ST, N, L, ncls, h, ldh, eps, labels,
                       E, zc, kld);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_cvae_latent_bwd(int N, int L, int ncls, const float* h, int ldh, const float* eps, const int64_t* labels, const float* dzc,
                                  int lddzc, float g_kld, const float* g_dev, float* dh, float* dE, void* stream) {
    MI_REQUIRE(N > 0 && L > 0 && ncls > 0 && h && eps && labels && dzc && dh && dE, "bad argument");
    MI_REQUIRE(ldh >= 2 * L && lddzc >= 2 * L, "ldh / lddzc < 2 L");
    MI_REQUIRE((size_t)N * L < (1ull << 29) && (size_t)ncls * L < (1ull << 29), "too many elements");
    const int nb_dh = nblk((size_t)N * L), nb_de = (ncls * L + TPB - 1) / TPB;
    hipLaunchKernelGGL(cvae_latent_bwd_kernel, dim3(nb_dh + nb_de), dim3(TPB), 0, ST, N, L, ncls, h, ldh, eps, labels, dzc, lddzc, g_kld, g_dev,
                       dh, dE, nb_dh);
    MI_LAUNCH_CHECK();
    return 0;
}
